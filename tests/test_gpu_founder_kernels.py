"""What the founder kernels write (pbwt_cut_trials_kernel, pbwt_cut_records_kernel in csrc/founder_kernels.hpp), compared value for value
with a plain pBWT (tests/pbwt_ref.py, pinned on the CPU by tests/test_pbwt_ref.py).

tests/test_gpu_founders.py compares the END of the pipeline -- cut positions after the host's score recurrence, matchings after its
sort and greedy assignment --, and both reduce the kernels' output many to one: a wrong class count on a pair that is not the optimum,
a pair too many that loses, rec_first_class outside a tie change nothing there.  Here v2m_pbwt_cut_trials,
v2m_pbwt_cut_trials_streamed and v2m_pbwt_cut_records are called through ctypes on chain graphs (one ALT edge per node) whose path
matrix, candidate and cut lists, chunkings and capacities are the test's own, with start states by definition (pbwt_ref.state_at),
and every output is compared exactly: the ordered pairs per candidate, trial_end, chunk_status, the per-cut records, the joined
classes in pBWT order.  Output arrays are pre-filled with a canary: everything past a chunk's last pair or joined class, and
everything that belongs to candidates and cuts outside the call's chunks, must still hold it.  A chunk's outputs are left
uncompared only where the REFERENCE says the kernel has to hand it back (more than 1024 bins at a candidate, or more pairs or
joined classes than the capacity); everywhere else chunk_status must be 0.

Wall times on an MI355X (one visit, product build): this module 16 s for its 77 tests (18 s with the interpreter's start), most of
it the reference on the CPU; the checked corpus of tests/test_gpu_checked_build.py 28.5 s per seed before its additions from this
module and 30.4 s after (its child's limit is 900 s).  The slice hand-over of the streamed form is covered here by one call of
4.6 million pairs (two pinned slices); the reference's side of it takes about 10 s.
"""

import ctypes as C
import os

import numpy as np
import pytest

import oracle
import pbwt_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CANARY32, CANARY64 = 0xCACACACA, 0xCACACACACACACACA
MAX_BINS = 1024                                                                # include/v2m_hip.h: more bins at one candidate and the chunk comes back


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	with v2m.Context(0) as c:                                                  # one context for the module: every case binds a graph of its own to it
		yield c


class Bound:
	"""A chain graph of bits.shape[1] edges with the path matrix bits[copy, edge] (padded to path_cols copy columns), uploaded to ctx.
	device_bind: the graph goes up without its matrix and the edge-by-copy form is bound from device memory (v2m_bind_path_matrix_device):
	the context's matrix is then its own line-aligned one, not the dense one of v2m_upload_graph."""

	def __init__(self, v2m, ctx, bits, path_cols=None, seed=0, device_bind=False):
		self.ctx, self.bits = ctx, bits
		self.n_edges = bits.shape[1]
		arrays, ref = R.chain_graph_arrays(self.n_edges, seed)
		rows, cols = R.round64(self.n_edges), path_cols or R.round64(bits.shape[0])
		og = oracle.graph_from_arrays(path_words=R.pack_paths(bits, rows, cols), path_rows=rows, path_cols=cols, **arrays)
		vg = v2m.VariantGraph.from_object(og)
		if device_bind:
			import torch
			vg.paths_by_chrom_copy_and_edge = None
			ctx.upload_graph(vg, ref)
			by_edge = R.pack_paths(bits.T, cols, rows)                              # one column of cols / 64 words per edge
			d_by_edge = torch.from_numpy(by_edge.view(np.int64)).cuda()
			torch.cuda.synchronize()
			ctx.bind_path_matrix_device(d_by_edge.data_ptr(), cols, rows)
			ctx.synchronize()                                                      # (the call is asynchronous and d_by_edge goes away here)
		else:
			ctx.upload_graph(vg, ref)
		self.aligned = [int(a) for a in arrays["aligned_positions"]]             # of node n = the node after n edges

	def candidates(self, edges):
		"""The sentinel and one candidate per entry of `edges` (ascending, repeats allowed), at the node after that many edges."""
		cand_edge = [0] + [int(e) for e in edges]
		return cand_edge, [self.aligned[e] for e in cand_edge]

	def states(self, n_copies, edges):
		s = [R.state_at(self.bits[:n_copies], int(e)) for e in edges]
		return s

	# ---- v2m_pbwt_cut_trials / _streamed ------------------------------------------------------------------------------------
	def trials(self, n_copies, min_distance, cand_edge, cand_aligned, chunk_first, capacity, streamed=False, sink_fails_at=None, states=None):
		"""Runs the call on start states by definition and compares everything it wrote with the reference.  Returns (rc, undone chunks
		as the reference predicts them, sink calls)."""
		from vcf2multialign_amd import _native as N
		n_chunks = len(chunk_first) - 1
		if states is None:
			states = self.states(n_copies, [cand_edge[f] if f < len(cand_edge) else 0 for f in chunk_first[:-1]])
		ce, ca, cf = np.array(cand_edge, dtype=np.uint32), np.array(cand_aligned, dtype=np.uint64), np.array(chunk_first, dtype=np.uint64)
		so = np.ascontiguousarray(np.concatenate([s[0] for s in states]), dtype=np.uint32)
		sd = np.ascontiguousarray(np.concatenate([s[1] for s in states]), dtype=np.uint32)
		pred = np.full(max(1, n_chunks * capacity), CANARY32, dtype=np.uint32)
		cls = np.full(max(1, n_chunks * capacity), CANARY32, dtype=np.uint32)
		end = np.full(len(ce), CANARY64, dtype=np.uint64)
		status = np.full(n_chunks, CANARY32, dtype=np.uint32)
		lib, calls = self.ctx._lib, []
		if streamed:
			def sink(user, chunk, chunk_status, p, c, n):
				take = lambda a: np.frombuffer((C.c_uint32 * n).from_address(a), dtype=np.uint32).copy() if n else np.zeros(0, dtype=np.uint32)
				calls.append((int(chunk), int(chunk_status), take(p), take(c)))
				return 7 if chunk == sink_fails_at else 0
			rc = lib.v2m_pbwt_cut_trials_streamed(self.ctx._h, n_copies, min_distance, len(ce), ce.ctypes.data, ca.ctypes.data, n_chunks, cf.ctypes.data,
				so.ctypes.data, sd.ctypes.data, capacity, end.ctypes.data, status.ctypes.data, N.TRIALS_SINK_FN(sink), None)
			if sink_fails_at is not None:
				assert rc == N.V2M_ERR_SINK and [c[0] for c in calls] == list(range(sink_fails_at + 1))
				assert b"trial sink returned 7 at chunk %d" % sink_fails_at in lib.v2m_last_error(self.ctx._h)
				return rc, None, calls
		else:
			rc = lib.v2m_pbwt_cut_trials(self.ctx._h, n_copies, min_distance, len(ce), ce.ctypes.data, ca.ctypes.data, n_chunks, cf.ctypes.data,
				so.ctypes.data, sd.ctypes.data, capacity, pred.ctypes.data, cls.ctypes.data, end.ctypes.data, status.ctypes.data)
		assert rc == N.V2M_OK, lib.v2m_last_error(self.ctx._h)
		if streamed:
			assert [c[0] for c in calls] == list(range(n_chunks))                 # one call per chunk, in chunk order
		undone = []
		for k in range(n_chunks):
			first, last = int(chunk_first[k]), int(chunk_first[k + 1])
			pairs, bins = R.walk_trials(self.bits, n_copies, cand_edge, cand_aligned, first, last, min_distance, self.n_edges, state=states[k])
			flat = [p for cand in pairs for p in cand]
			where = "chunk %d (candidates %d .. %d)" % (k, first, last)
			if any(b > MAX_BINS for b in bins) or len(flat) > capacity:
				undone.append(k)
				assert 1 == status[k], where
				got_pred, got_cls = (calls[k][2], calls[k][3]) if streamed else (pred[k * capacity:k * capacity], cls[k * capacity:k * capacity])
				assert 0 == len(got_pred) and 0 == len(got_cls), where            # (streamed: 0 pairs for a chunk left undone)
				if streamed:
					assert 1 == calls[k][1], where
				n = 0
			else:
				assert 0 == status[k], where
				n = len(flat)
				got_pred, got_cls = (calls[k][2], calls[k][3]) if streamed else (pred[k * capacity:k * capacity + n], cls[k * capacity:k * capacity + n])
				if streamed:
					assert 0 == calls[k][1] and n == len(got_pred) == len(got_cls), where
				assert got_pred.tolist() == [p for p, _ in flat], where
				assert got_cls.tolist() == [c for _, c in flat], where
				assert end[first:last].tolist() == np.cumsum([len(cand) for cand in pairs]).tolist(), where
			if not streamed:                                                      # nothing past the chunk's last pair
				assert (pred[k * capacity + n:(k + 1) * capacity] == CANARY32).all() and (cls[k * capacity + n:(k + 1) * capacity] == CANARY32).all(), where
		# trial_end of candidates outside this call's chunks
		assert (end[:int(chunk_first[0])] == CANARY64).all() and (end[int(chunk_first[-1]):] == CANARY64).all()
		return rc, undone, calls

	# ---- v2m_pbwt_cut_records ------------------------------------------------------------------------------------------------
	def records(self, n_copies, cut_edge, chunk_first_cut, capacity, start_edge=None, expect_rc=None):
		from vcf2multialign_amd import _native as N
		n_chunks = len(chunk_first_cut) - 1
		if start_edge is None:
			start_edge = [cut_edge[f - 1] for f in chunk_first_cut[:-1]]
		states = self.states(n_copies, start_edge)
		cu, cf, se = np.array(cut_edge, dtype=np.uint32), np.array(chunk_first_cut, dtype=np.uint64), np.array(start_edge, dtype=np.uint32)
		so = np.ascontiguousarray(np.concatenate([s[0] for s in states]), dtype=np.uint32)
		sd = np.ascontiguousarray(np.concatenate([s[1] for s in states]), dtype=np.uint32)
		pools = [np.full(max(1, n_chunks * capacity), CANARY32, dtype=np.uint32) for _ in range(3)]
		pool_end = np.full(len(cu), CANARY64, dtype=np.uint64)
		recs = [np.full(len(cu), CANARY32, dtype=np.uint32) for _ in range(3)]   # distinct, first_class, first_is_ref
		status = np.full(n_chunks, CANARY32, dtype=np.uint32)
		lib = self.ctx._lib
		rc = lib.v2m_pbwt_cut_records(self.ctx._h, n_copies, len(cu), cu.ctypes.data, n_chunks, cf.ctypes.data, se.ctypes.data, so.ctypes.data, sd.ctypes.data,
			capacity, pools[0].ctypes.data, pools[1].ctypes.data, pools[2].ctypes.data, pool_end.ctypes.data, recs[0].ctypes.data, recs[1].ctypes.data, recs[2].ctypes.data,
			status.ctypes.data)
		if expect_rc is not None:
			assert rc == expect_rc
			assert all((a == CANARY32).all() for a in pools + recs + [status]) and (pool_end == CANARY64).all()   # refused before anything was written
			return rc, None
		assert rc == N.V2M_OK, lib.v2m_last_error(self.ctx._h)
		undone = []
		for k in range(n_chunks):
			first, last = int(chunk_first_cut[k]), int(chunk_first_cut[k + 1])
			want = R.walk_records(self.bits, n_copies, cut_edge, first, last, start_edge=start_edge[k], state=states[k])
			flat = [j for rec in want for j in (rec["joined"] or [])]
			where = "chunk %d (cuts %d .. %d)" % (k, first, last)
			n = 0
			if len(flat) > capacity:
				undone.append(k)
				assert 1 == status[k], where
			else:
				assert 0 == status[k], where
				n = len(flat)
				for which, pool in enumerate(pools):
					assert pool[k * capacity:k * capacity + n].tolist() == [j[which] for j in flat], (where, which)
				assert pool_end[first:last].tolist() == np.cumsum([len(rec["joined"] or []) for rec in want]).tolist(), where
				for name, got in zip(("distinct", "first_class", "first_is_ref"), recs):
					assert got[first:last].tolist() == [rec[name] for rec in want], (where, name)
			for pool in pools:
				assert (pool[k * capacity + n:(k + 1) * capacity] == CANARY32).all(), where
		lo, hi = int(chunk_first_cut[0]), int(chunk_first_cut[-1])
		for a, canary in [(pool_end, CANARY64)] + [(r, CANARY32) for r in recs]:
			assert (a[:lo] == canary).all() and (a[hi:] == canary).all()
		return rc, undone


def _ascending(rng, n, n_edges, repeats=0):
	"""n edge counts out of 0 .. n_edges, ascending, with `repeats` of them doubled."""
	picked = sorted(int(e) for e in rng.choice(n_edges + 1, size=min(n, n_edges + 1), replace=False))
	for e in rng.choice(picked, size=min(repeats, len(picked)), replace=False):
		picked.append(int(e))
	return sorted(picked)


def _both_kernels(b, n_copies, rng, n_candidates=9, n_cuts=7, min_distance=0, capacity=None):
	"""A few candidates in three chunks and a few cuts in two, all chunks done."""
	cand_edge, cand_aligned = b.candidates([0] + _ascending(rng, n_candidates, b.n_edges, repeats=1))
	n = len(cand_edge)
	_, undone, _ = b.trials(n_copies, min_distance, cand_edge, cand_aligned, [1, 1 + n // 3, 1 + 2 * n // 3, n], capacity or n * (MAX_BINS + 2))
	assert [] == undone
	inner = [e for e in _ascending(rng, n_cuts, b.n_edges) if 0 < e < b.n_edges]
	cut_edge = [0] + inner + [b.n_edges]
	_, undone = b.records(n_copies, cut_edge, [1, 1 + len(cut_edge) // 2, len(cut_edge)], len(cut_edge) * n_copies)
	assert [] == undone


SEAMS = sorted({1, 2, 63, 64, 65, 1023, 1024, 1025} | {1024 * p + d for p in (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 20) for d in (-1, 0, 1) if 1024 * p + d <= 20480})
SMALL_SEAMS = [n for n in SEAMS if n < 2100]


@pytest.mark.parametrize("n_copies", SEAMS)
def test_copy_counts_at_every_seam(v2m, ctx, n_copies):
	"""Every copy count where a thread's last copy, a wave, the workgroup or an instantiation (1 .. 8, 10, 12, 16, 20 copies per thread; class
	arrays in LDS up to 12 288 copies, in device memory above) begins or ends, with dense, sparse and many-identical-copies bits."""
	n_edges = 150 if n_copies > 2100 else 260
	for name in ("dense", "sparse", "clones"):
		rng = np.random.default_rng([n_copies, R.FAMILIES.index(name)])
		_both_kernels(Bound(v2m, ctx, R.family(name, n_copies, n_edges, seed=1)), n_copies, rng)


@pytest.mark.parametrize("path_cols", [12352, 20480])
@pytest.mark.parametrize("n_copies", [1, 5, 1000])
def test_few_copies_under_a_wide_matrix(v2m, ctx, n_copies, path_cols):
	"""The instantiation follows the bound matrix's columns, not the copies walked: most threads hold no copy at all, the last one that
	holds any has slots past its last copy (pbwt_step's "counts as a copy of class 1").  The other columns hold bits of their own."""
	bits = R.family("dense", path_cols, 100, seed=2)
	b = Bound(v2m, ctx, bits, path_cols=path_cols)
	_both_kernels(b, n_copies, np.random.default_rng([n_copies, path_cols]))


@pytest.mark.parametrize("name,n_copies,per", [(name, n, per) for n, per in ((130, 1), (2500, 3), (16400, 20)) for name in R.FAMILIES
	if n < 3000 or name not in ("identity", "genotypes")])                     # (far more copies than edges leave these two nearly constant)
def test_matrix_families(v2m, ctx, name, n_copies, per):
	"""Columns chosen for the scans: constant ones (first and last among them), ones that are exactly one wave's or one 16-lane row's
	copies, alternating blocks of a thread's length, the identity (values spread over all earlier candidates), genotype-like bits."""
	n_edges = 200 if n_copies < 3000 else 100
	bits = R.family(name, n_copies, n_edges, seed=3, per=per)
	_both_kernels(Bound(v2m, ctx, bits), n_copies, np.random.default_rng([n_copies, R.FAMILIES.index(name)]), n_candidates=25, n_cuts=12)


def test_bin_limits(v2m, ctx):
	"""The identity family with a candidate at every node: candidate c has c - 1 bins.  A chunk that ends at the candidate with exactly
	1024 comes back done, with exact pairs; one that reaches the candidate with 1025 comes back undone, and so does nothing else."""
	n = 1030
	b = Bound(v2m, ctx, R.family("identity", n, n))
	cand_edge, cand_aligned = b.candidates(range(n + 1))
	capacity = 40 * 1100
	_, undone, _ = b.trials(n, 0, cand_edge, cand_aligned, [990, 1010, 1026, 1026, 1027, 1030], capacity)     # chunk 1 ends at 1025 (1024 bins), chunk 3 is 1026 (1025 bins)
	assert [3, 4] == undone
	_, undone, _ = b.trials(n, 0, cand_edge, cand_aligned, [1000, 1027], capacity)
	assert [0] == undone
	_, undone, _ = b.trials(n, 0, cand_edge, cand_aligned, [1, 400, 800, 1026], 1026 * 1026)                   # everything up to the limit, three chunks
	assert [] == undone


def test_hash_collisions_in_both_tables(v2m, ctx):
	"""Bins 1 and 1293 share a slot of the 2048-slot table (more than 8 copies per thread), 2 and 2586 one of the 4096-slot table: five
	copies whose values point to exactly these four candidates (tests/test_pbwt_ref.py), under a narrow and under a wide matrix."""
	bits, n_edges, cand_edge = R.collision_case()
	for path_cols in (64, 8192 + 64):
		wide = np.zeros((path_cols, n_edges), dtype=bool)
		wide[:5] = bits
		wide[5:] = R.family("sparse", path_cols - 5, n_edges, seed=4)
		b = Bound(v2m, ctx, wide, path_cols=path_cols)
		_, undone, _ = b.trials(5, 0, cand_edge, [b.aligned[e] for e in cand_edge], [2580, 2590, n_edges + 1], 200)
		assert [] == undone


def test_capacities(v2m, ctx):
	"""Exactly what a chunk needs: done.  One less: undone, and the chunks beside it untouched (the comparison of every chunk's region
	and the canary behind it).  Capacity 0 with chunks that produce nothing."""
	n_copies, n_edges = 700, 300
	b = Bound(v2m, ctx, R.family("genotypes", n_copies, n_edges, seed=5))
	rng = np.random.default_rng(5)
	cand_edge, cand_aligned = b.candidates([0] + _ascending(rng, 40, n_edges))
	chunk_first = [1, 9, 20, 33, len(cand_edge)]
	need = [sum(len(c) for c in R.walk_trials(b.bits, n_copies, cand_edge, cand_aligned, f, l, 0, n_edges)[0]) for f, l in zip(chunk_first, chunk_first[1:])]
	fullest = int(np.argmax(need))
	assert need[fullest] > max(n for k, n in enumerate(need) if k != fullest)   # (so that one less leaves the others room)
	for streamed in (False, True):
		assert [] == b.trials(n_copies, 0, cand_edge, cand_aligned, chunk_first, need[fullest], streamed=streamed)[1]
		assert [fullest] == b.trials(n_copies, 0, cand_edge, cand_aligned, chunk_first, need[fullest] - 1, streamed=streamed)[1]
	# the candidate at edge 0 in the state before the first edge has nothing to try: no pair, capacity 0 is enough; the next chunk needs more
	assert [] == b.trials(n_copies, 0, cand_edge, cand_aligned, [1, 2, 2], 0)[1]
	assert [1] == b.trials(n_copies, 0, cand_edge, cand_aligned, [1, 2, 5], 0)[1]

	cut_edge = [0] + [e for e in _ascending(rng, 14, n_edges) if 0 < e < n_edges] + [n_edges]
	chunk_first_cut = [1, 5, 9, len(cut_edge)]
	need = [sum(len(r["joined"] or []) for r in R.walk_records(b.bits, n_copies, cut_edge, f, l)) for f, l in zip(chunk_first_cut, chunk_first_cut[1:])]
	fullest = int(np.argmax(need))
	assert need[fullest] > max(n for k, n in enumerate(need) if k != fullest)
	assert [] == b.records(n_copies, cut_edge, chunk_first_cut, need[fullest])[1]
	assert [fullest] == b.records(n_copies, cut_edge, chunk_first_cut, need[fullest] - 1)[1]
	assert [] == b.records(n_copies, cut_edge, [1, 2, 2], 0)[1]                # cut 1 has no two-block span: no joined class
	assert [1] == b.records(n_copies, cut_edge, [1, 2, 4], 0)[1]


def test_chunkings_the_host_never_makes(v2m, ctx):
	n_copies, n_edges = 1500, 400
	b = Bound(v2m, ctx, R.family("genotypes", n_copies, n_edges, seed=6))
	rng = np.random.default_rng(6)
	# the sentinel and the first candidate share edge 0, as in every real run; two more candidates share an edge count further on
	cand_edge, cand_aligned = b.candidates([0] + _ascending(rng, 60, n_edges, repeats=3))
	n = len(cand_edge)
	capacity = n * 300
	for chunk_first in (
		[1, n],                                                                # one chunk for everything, from the state before the first edge (the only one with "no match yet")
		list(range(1, n + 1)),                                                 # a chunk per candidate
		[1, 1, 7, 7, 7, 30, n, n],                                             # empty chunks between full ones
		[5, 20],                                                               # candidates before and behind the call's chunks keep their trial_end
	):
		assert [] == b.trials(n_copies, 0, cand_edge, cand_aligned, chunk_first, capacity)[1]
	# 300 chunks in one call: more workgroups than the card has compute units
	cand_edge, cand_aligned = b.candidates(range(n_edges + 1))
	assert [] == b.trials(n_copies, 3, cand_edge, cand_aligned, list(range(1, 302)), MAX_BINS + 2)[1]

	inner = [e for e in _ascending(rng, 30, n_edges, repeats=2) if 0 < e < n_edges]   # two cuts twice with no edge between them
	cut_edge = [0, 0] + inner + [n_edges]                                              # ... and cut 1 at edge 0, beside node 0
	assert all(cut_edge[j] != cut_edge[j - 2] for j in range(2, len(cut_edge)))
	m = len(cut_edge)
	for chunk_first_cut in ([1, m], list(range(1, m + 1)), [1, 1, 4, 4, 4, 19, m, m], [3, 11]):
		assert [] == b.records(n_copies, cut_edge, chunk_first_cut, m * n_copies)[1]
	# start states well before the cut in front of the chunk's first one: the kernel walks there by itself
	chunk_first_cut = [2, 9, 20, m]
	start_edge = [max(0, cut_edge[f - 1] - back) for f, back in zip(chunk_first_cut, (10 ** 6, 37, 1))]
	assert [] == b.records(n_copies, cut_edge, chunk_first_cut, m * n_copies, start_edge=start_edge)[1]
	cut_edge = list(range(n_edges + 1))
	assert [] == b.records(n_copies, cut_edge, list(range(1, 302)), n_copies)[1]


def test_min_distance(v2m, ctx):
	"""0, exactly the distance between two candidates, one more, and more than the whole alignment (only the final pair is left)."""
	n_copies, n_edges = 300, 200
	b = Bound(v2m, ctx, R.family("dense", n_copies, n_edges, seed=7))
	cand_edge, cand_aligned = b.candidates(range(n_edges + 1))
	n = len(cand_edge)
	exact = cand_aligned[150] - cand_aligned[141]
	with_it = R.walk_trials(b.bits, n_copies, cand_edge, cand_aligned, 150, 151, exact, n_edges)[0][0]
	without = R.walk_trials(b.bits, n_copies, cand_edge, cand_aligned, 150, 151, exact + 1, n_edges)[0][0]
	assert len(without) < len(with_it)                                         # (the limit decides a pair of candidate 150)
	for min_distance in (0, exact, exact + 1, cand_aligned[-1] + 1):
		assert [] == b.trials(n_copies, min_distance, cand_edge, cand_aligned, [1, 100, 150, 151, n], n * 64)[1]


def test_streamed_form(v2m, ctx):
	"""One sink call per chunk in chunk order with the array form's pairs; 0 pairs and status 1 for a chunk left undone; a sink that
	returns 7 at chunk 2 ends the call with V2M_ERR_SINK and leaves the ctx usable."""
	n_copies, n_edges = 1100, 300
	b = Bound(v2m, ctx, R.family("genotypes", n_copies, n_edges, seed=8))
	cand_edge, cand_aligned = b.candidates(range(n_edges + 1))
	n = len(cand_edge)
	chunk_first = [1, 40, 40, 120, 250, n]
	assert [] == b.trials(n_copies, 2, cand_edge, cand_aligned, chunk_first, n * 400, streamed=True)[1]
	assert [] == b.trials(n_copies, 2, cand_edge, cand_aligned, chunk_first, n * 400)[1]
	need = [sum(len(c) for c in R.walk_trials(b.bits, n_copies, cand_edge, cand_aligned, f, l, 2, n_edges)[0]) for f, l in zip(chunk_first, chunk_first[1:])]
	capacity = sorted(need)[-2]                                                 # the chunk with the most pairs does not fit
	assert [int(np.argmax(need))] == b.trials(n_copies, 2, cand_edge, cand_aligned, chunk_first, capacity, streamed=True)[1]
	from vcf2multialign_amd import _native as N
	rc, _, calls = b.trials(n_copies, 2, cand_edge, cand_aligned, chunk_first, n * 400, streamed=True, sink_fails_at=2)
	assert rc == N.V2M_ERR_SINK and 3 == len(calls)
	assert [] == b.trials(n_copies, 2, cand_edge, cand_aligned, chunk_first, n * 400, streamed=True)[1]      # the ctx is as usable as before
	assert [] == b.records(n_copies, [0, 50, 120, n_edges], [1, 4], 4 * n_copies)[1]


def test_streamed_form_over_more_than_one_pinned_slice(v2m, ctx):
	"""More than 4 Mi pairs in one call: the chunks come back through both pinned slots in turn (v2m_hip.hip: slot_pairs).  900 copies of
	the identity family wrapped around (column e is set for copy e mod 900) keep about 900 bins and pairs at every one of 5600 candidates."""
	n_copies, n_edges = 900, 5600
	b = Bound(v2m, ctx, np.arange(n_copies)[:, None] == (np.arange(n_edges)[None, :] % n_copies))
	cand_edge, cand_aligned = b.candidates(range(n_edges + 1))
	chunk_first = [1] + [700 * k for k in range(1, 8)] + [len(cand_edge)]
	_, undone, calls = b.trials(n_copies, 0, cand_edge, cand_aligned, chunk_first, 700 * 1000, streamed=True)
	assert [] == undone
	pairs = [len(c[2]) for c in calls]
	assert sum(pairs) > 4 << 20 and sum(pairs[:7]) <= 4 << 20                  # seven chunks fill the first slice, the eighth travels in the second


def test_cut_lists_the_search_never_produces(v2m, ctx):
	"""Cut positions given by the user reach the kernel unchecked by the search.  Two cuts in a row with no ALT edge between them give a
	block without classes (the reference's loop, restated without its assertions, and the kernel agree on every value); three in a row
	leave a two-block span in which no copy starts a class: the reference asserts (founder_sequence_greedy_output.cc:245), the
	library refuses the list before it launches anything."""
	from vcf2multialign_amd import _native as N
	n_copies, n_edges = 260, 120
	b = Bound(v2m, ctx, R.family("dense", n_copies, n_edges, seed=9))
	assert [] == b.records(n_copies, [0, 30, 30, 77, 77, n_edges, n_edges], [1, 3, 7], 7 * n_copies)[1]
	for cut_edge in ([0, 30, 30, 30, n_edges], [0, 0, 0, n_edges], [0, 30, n_edges, n_edges, n_edges]):
		with pytest.raises(ValueError):
			R.walk_records(b.bits, n_copies, cut_edge, 1, len(cut_edge))
		b.records(n_copies, cut_edge, [1, len(cut_edge)], 5 * n_copies, expect_rc=N.V2M_ERR_INVALID_ARGUMENT)
		assert b"no ALT edge between them" in ctx._lib.v2m_last_error(ctx._h)
	assert [] == b.records(n_copies, [0, 30, 77, n_edges], [1, 4], 4 * n_copies)[1]


def _write_cuts(path, cuts):
	from vcf2multialign_amd import host
	host.write_cut_positions(str(path), cuts, 0, 5)


def test_cli_refuses_hand_written_cut_lists(tmp_path):
	"""--input-cut-positions with a repeated node, a node past the graph, a list that goes back, one that does not start at node 0 or does
	not end at the last node, one with a block that holds no ALT edge: an error message, no crash and no A2M file."""
	import subprocess
	import synth
	cli = os.path.join(os.path.dirname(HERE), "vcf2multialign_amd", "bin", "vcf2multialign")
	g = synth.build_case(tmp_path, 66, 20000, 300, 5)
	common = ["-F", "3", "-r", str(tmp_path / "synth.fa"), "-a", str(tmp_path / "synth.vcf"), "-c", "1"]
	good = tmp_path / "good.bin"
	r = subprocess.run([cli] + common + ["-d", "20", "-s", str(tmp_path / "good.a2m"), "-t", str(good)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
	assert 0 == r.returncode, r.stderr.decode()
	from vcf2multialign_amd import host
	cuts = host.read_cut_positions(str(good))[0]
	last = g.node_count - 1
	assert len(cuts) >= 4 and 0 == cuts[0] and last == cuts[-1]
	csum = g.alt_edge_count_csum
	flat = next(n for n in range(1, last - 1) if csum[n] == csum[n + 1] and 0 < csum[n] < csum[last])   # two nodes with no ALT edge between them
	for name, bad, message in (
		("repeated", cuts[:2] + cuts[1:], b"does not lie after"),
		("past_the_end", cuts[:-1] + [last + 5], b"lies outside the graph"),
		("descending", [cuts[0], cuts[2], cuts[1]] + cuts[3:], b"does not lie after"),
		("not_from_node_0", cuts[1:], b"must be node 0"),
		("not_to_the_last_node", cuts[:-1], b"must be the last node"),
		("block_without_an_edge", [0, flat, flat + 1, last], b"without any ALT edge"),
	):
		_write_cuts(tmp_path / (name + ".bin"), bad)
		out = tmp_path / (name + ".a2m")
		r = subprocess.run([cli] + common + ["-s", str(out), "--input-cut-positions=" + str(tmp_path / (name + ".bin"))], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
		assert 1 == r.returncode and b"ERROR: cut position" in r.stderr and message in r.stderr, (name, r.returncode, r.stderr.decode())
		assert not out.exists(), name
