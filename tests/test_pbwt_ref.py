"""tests/pbwt_ref.py pinned on the CPU, without the code under test: its pBWT step against the state by definition, its pairs through
the score recurrence against the reference's own cut positions (tests/golden/reference_goldens.json) and the oracle's literal
search, its joined classes through a literal greedy assignment against the reference's matchings -- and the constructions
tests/test_gpu_founder_kernels.py relies on really reach the edges they aim at (bin limits, hash collisions, minimum distances)."""

import json
import os

import numpy as np
import pytest

import oracle
import pbwt_ref as R
import synth

HERE = os.path.dirname(os.path.abspath(__file__))


def _bits_of_graph(og):
	return R.unpack_paths(og.paths_by_chrom_copy_and_edge, og.path_rows, og.path_cols)[:og.total_chromosome_copies, :og.edge_count]


def _states_equal(a, b):
	return [int(x) for x in a[0]] == [int(x) for x in b[0]] and [int(x) for x in a[1]] == [int(x) for x in b[1]]


@pytest.mark.parametrize("n_copies", [1, 2, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("name", ["dense", "sparse", "clones", "constant_columns", "lane_blocks", "alternating", "identity"])
def test_stepping_gives_the_state_by_definition(n_copies, name):
	n_edges = 40
	bits = R.family(name, n_copies, n_edges, seed=11)
	state = R.initial_state(n_copies)
	for k in range(n_edges + 1):
		assert _states_equal(state, R.state_at_literal(bits, k)), k
		assert _states_equal(state, R.state_at(bits, k)), k
		if k < n_edges:
			state = R.step(state[0], state[1], bits[:, k], k)
	assert 1 == n_copies or 0 not in state[1]                                   # "no match yet" does not outlive the first edge


def test_stepping_gives_the_state_by_definition_2000_copies():
	n_copies, n_edges = 2003, 24
	for name in ("dense", "clones"):
		bits = R.family(name, n_copies, n_edges, seed=12)
		state = R.initial_state(n_copies)
		for k in range(n_edges + 1):
			assert _states_equal(state, R.state_at(bits, k)), (name, k)
			if k in (0, 1, 7, n_edges):
				assert _states_equal(state, R.state_at_literal(bits, k)), (name, k)
			if k < n_edges:
				state = R.step(state[0], state[1], bits[:, k], k)


@pytest.mark.parametrize("n_copies", [1, 2, 3, 64, 65, 130, 2003])
@pytest.mark.parametrize("name", ["dense", "sparse", "clones", "constant_columns", "identity"])
def test_vectorised_forms_equal_the_literal_ones(n_copies, name):
	"""step_np / records_at_np, which the GPU module walks its thousands of copies with, against the literal loops: states after every
	edge, pairs at every candidate, records at every cut -- chunked from states by definition and in one go from the first edge."""
	n_edges = 30
	bits = R.family(name, n_copies, n_edges, seed=21)
	state = R.initial_state(n_copies)
	for k in range(n_edges):
		fast = R.step_np(state[0], state[1], bits[:, k], k)
		state = R.step(state[0], state[1], bits[:, k], k)
		assert _states_equal(state, fast), k
	arrays, _ = R.chain_graph_arrays(n_edges, seed=2)
	cand_edge, _, cand_aligned = R.every_node_candidates(n_edges, arrays["aligned_positions"])
	whole = R.walk_trials(bits, n_copies, cand_edge, cand_aligned, 1, len(cand_edge), 3, n_edges, state=R.initial_state(n_copies), literal=True)
	assert R.walk_trials(bits, n_copies, cand_edge, cand_aligned, 1, len(cand_edge), 3, n_edges, state=R.initial_state(n_copies)) == whole
	for first, end in ((1, 2), (2, 9), (9, 9), (9, len(cand_edge))):
		assert R.walk_trials(bits, n_copies, cand_edge, cand_aligned, first, end, 3, n_edges) == (whole[0][first - 1:end - 1], whole[1][first - 1:end - 1])
	cut_edge = [0, 0, 3, 4, 4, 11, 30]                                          # (consecutive cuts with no edge between them among them)
	whole = R.walk_records(bits, n_copies, cut_edge, 1, len(cut_edge), start_edge=0, state=R.initial_state(n_copies), literal=True)
	assert R.walk_records(bits, n_copies, cut_edge, 1, len(cut_edge), start_edge=0, state=R.initial_state(n_copies)) == whole
	for first, end in ((1, 3), (3, 4), (4, 7)):
		assert R.walk_records(bits, n_copies, cut_edge, first, end) == whole[first - 1:end - 1]
		assert R.walk_records(bits, n_copies, cut_edge, first, end, start_edge=max(0, cut_edge[first - 1] - 3)) == whole[first - 1:end - 1]


def test_three_cuts_with_no_edge_between_them_are_refused():
	"""cut_edge[j] == cut_edge[j - 2]: no copy starts a class of the two-block span, and the reference stops at its
	libbio_assert(!joined_path_eq_classes.empty()) (founder_sequence_greedy_output.cc:245)."""
	bits = R.family("dense", 9, 12, seed=1)
	for literal in (True, False):
		with pytest.raises(ValueError):
			R.walk_records(bits, 9, [0, 5, 5, 5, 12], 1, 5, literal=literal)
		assert 4 == len(R.walk_records(bits, 9, [0, 5, 5, 8, 12], 1, 5, literal=literal))


def _search(og, bits, min_distance):
	cand_edge, cand_node, cand_aligned = R.candidates_of_graph(og.alt_edge_targets, og.alt_edge_count_csum, og.aligned_positions)
	pairs, _ = R.walk_trials(bits, bits.shape[0], cand_edge, cand_aligned, 1, len(cand_edge), min_distance, og.edge_count, state=R.initial_state(bits.shape[0]))
	return R.cut_positions_from_trials(pairs, cand_edge, cand_node, bits.shape[0], og.node_count)


def _founder_cases():
	with open(os.path.join(HERE, "golden", "reference_goldens.json")) as f:
		return json.load(f)["founder_sequences"]


@pytest.mark.parametrize("case", _founder_cases(), ids=lambda c: c["vcf"] + "+" + c["fasta"])
def test_reference_goldens(case, fixtures_dir):
	"""The reference's own test (tests/founder_sequences.cc:130-186): cut positions from the pairs, matchings from the joined classes."""
	d = os.path.join(fixtures_dir, "founder-sequences")
	og = oracle.build_variant_graph(os.path.join(d, case["fasta"]), os.path.join(d, case["vcf"]), case["chromosome"])
	bits = _bits_of_graph(og)
	cuts, _ = _search(og, bits, case["minimum_distance"])
	assert cuts == case["cut_positions"]
	cut_edge = [int(og.alt_edge_count_csum[n]) for n in cuts]
	records = R.walk_records(bits, bits.shape[0], cut_edge, 1, len(cuts), state=R.initial_state(bits.shape[0]), start_edge=0)
	# (at most a handful of joined classes per cut: every std::sort sorts those by insertion, which keeps equal sizes in order)
	assert R.greedy_assignment(records, bits.shape[0], case["founder_count"]) == case["assigned_samples_column_major"]
	# the chunked form of the walk (start states by definition, a chunk per cut) gives the same records
	for j in range(1, len(cuts)):
		assert R.walk_records(bits, bits.shape[0], cut_edge, j, j + 1) == records[j - 1:j]
		assert R.walk_records(bits, bits.shape[0], cut_edge, j, j + 1, start_edge=0, state=R.initial_state(bits.shape[0])) == records[j - 1:j]


@pytest.mark.parametrize("seed,ref_len,n_variants,n_samples,kw", [
	(1, 3000, 120, 6, dict()),
	(2, 5000, 400, 9, dict(multi_allelic=0.3)),
	(3, 20000, 900, 40, dict(mix=(0.6, 0.2, 0.2))),
	(4, 8000, 300, 3, dict(density=0.5)),
	(5, 8000, 300, 70, dict(density=0.02)),
	(6, 60000, 500, 12, dict(long_every=50)),
	(7, 2000, 60, 1, dict(ploidy=1)),
	(8, 30000, 2500, 33, dict(multi_allelic=0.1, mix=(0.7, 0.15, 0.15))),
], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_random_graphs_against_the_oracle(tmp_path, seed, ref_len, n_variants, n_samples, kw):
	"""The random graphs of test_gpu_founders.py::test_random_inputs: cut positions and score of the oracle's literal search, and its
	matchings where the order of joined classes of the same size is not left open by std::sort."""
	rng = np.random.default_rng(1000 + seed)
	ref = synth.random_reference(rng, ref_len)
	recs = synth.random_records(rng, ref, n_variants, n_samples, **kw)
	fa, vcf = synth.write_inputs(str(tmp_path), ref, recs, n_samples)
	og = oracle.build_variant_graph(fa, vcf, "1")
	bits = _bits_of_graph(og)
	n_copies = bits.shape[0]
	cand_edge, cand_node, cand_aligned = R.candidates_of_graph(og.alt_edge_targets, og.alt_edge_count_csum, og.aligned_positions)
	# one walk over the edges, the pairs per minimum distance from the divergence values it leaves at the candidates
	order, div = R.initial_state(n_copies)
	divs, edge = [], 0
	for c in range(1, len(cand_edge)):
		for edge in range(edge, cand_edge[c]):
			order, div = R.step(order, div, bits[:, edge], edge)
		edge = cand_edge[c]
		divs.append(div)
	for min_distance in (0, 10, 50, 1000, 10 * ref_len):
		pairs = [R.trials_at(divs[c - 1], cand_edge, cand_aligned, c, min_distance, og.edge_count)[0] for c in range(1, len(cand_edge))]
		got = R.cut_positions_from_trials(pairs, cand_edge, cand_node, n_copies, og.node_count)
		want = og.find_founders(2, min_distance)
		assert (got is None) == (want is None), min_distance
		if want is not None:
			assert got[0] == want[0] and got[1] == want[2], min_distance
			if 50 == min_distance and len(want[0]) > 2:
				cut_edge = [int(og.alt_edge_count_csum[n]) for n in want[0]]
				records = R.walk_records(bits, n_copies, cut_edge, 1, len(cut_edge), start_edge=0, state=R.initial_state(n_copies))
				# (the oracle is built with libstdc++, whose std::sort sorts up to 16 elements by insertion alone, which keeps equal
				# sizes in order like greedy_assignment's stable sort; seeds 1 and 5 stay below that, the others have ties in longer lists)
				if not R.has_size_ties(records) or max(len(rec["joined"] or []) for rec in records) <= 16:
					assert R.greedy_assignment(records, n_copies, 2) == want[1]
					assert seed in (1, 5)
				else:
					assert seed in (2, 3, 8)


@pytest.mark.parametrize("name,n_copies,n_edges", [("dense", 40, 90), ("clones", 130, 60), ("identity", 40, 40), ("genotypes", 66, 80), ("lane_blocks", 200, 50)])
def test_chain_graphs_against_the_oracle(name, n_copies, n_edges):
	"""The chain graphs of the GPU module, with path matrices of the test's own: the reference's pairs give the oracle's cut positions."""
	arrays, _ = R.chain_graph_arrays(n_edges, seed=3)
	bits = R.family(name, n_copies, n_edges, seed=5)
	rows, cols = R.round64(n_edges), R.round64(n_copies)
	og = oracle.graph_from_arrays(path_words=R.pack_paths(bits, rows, cols), path_rows=rows, path_cols=cols,
		sample_names=["S%d" % i for i in range(n_copies)], ploidy_csum=np.arange(n_copies + 1), **arrays)
	assert R.candidates_of_graph(og.alt_edge_targets, og.alt_edge_count_csum, og.aligned_positions) == R.every_node_candidates(n_edges, arrays["aligned_positions"])
	for min_distance in (0, 7, 40, 10 ** 6):
		got = _search(og, bits, min_distance)
		want = og.find_founders(2, min_distance)
		assert want is not None and got[0] == want[0] and got[1] == want[2], min_distance


# ---- the constructions of tests/test_gpu_founder_kernels.py ----------------------------------------------------------------------

def test_identity_family_spreads_its_values_over_all_earlier_candidates():
	"""With a candidate at every node the bins of candidate c (the sentinel is candidate 0) are c - 1, and its pairs (c - 1, 2),
	(c - 2, 3), ...: every pair carries a class count of its own, so any slot or sum error of the kernel shows."""
	n = 40
	arrays, _ = R.chain_graph_arrays(n)
	cand_edge, _, cand_aligned = R.every_node_candidates(n, arrays["aligned_positions"])
	pairs, bins = R.walk_trials(R.family("identity", n, n), n, cand_edge, cand_aligned, 1, len(cand_edge), 0, n)
	for c in range(2, n):
		assert bins[c - 1] == c - 1
		assert pairs[c - 1][:c - 2] == [(c - 1 - i, 2 + i) for i in range(c - 2)] and len(pairs[c - 1]) == c - 1


def bin_limit_case():
	"""1030 copies of the identity family, a candidate at every node: (bits, n_copies, n_edges, arrays, candidates, bins per candidate)."""
	n = 1030
	arrays, ref = R.chain_graph_arrays(n)
	cands = R.every_node_candidates(n, arrays["aligned_positions"])
	bits = R.family("identity", n, n)
	# the bins by definition, candidate by candidate (the step-by-step walk of 1030 x 1030 copies is left to the GPU test's reference run)
	bins = [R.trials_at(R.state_at(bits, cands[0][c])[1], cands[0], cands[2], c, 0, n)[1] for c in (1024, 1025, 1026)]
	return bits, n, arrays, cands, bins


def test_bin_limit_family_hits_1023_1024_and_1025_bins():
	_, _, _, _, bins = bin_limit_case()
	assert bins == [1023, 1024, 1025]


def test_collisions_in_both_hash_tables():
	"""Consecutive keys never share a slot of the kernels' multiplicative hash (the first two that do are 1 and 1293 with 2048 slots,
	2 and 2586 with 4096), so the GPU module brings a case of its own whose bins at one candidate hold both pairs: linear probing
	is on the path in both tables."""
	assert R.hash_slot(1, 2048) == R.hash_slot(1293, 2048) and R.hash_slot(2, 4096) == R.hash_slot(2586, 4096)
	for slots in (2048, 4096):
		assert len({R.hash_slot(k, slots) for k in range(1100)}) == 1100
	bits, n_edges, cand_edge = R.collision_case()
	for c in (2590, n_edges):
		assert R.bin_keys_at(R.state_at(bits, cand_edge[c])[1], cand_edge, c, n_edges) == [1, 2, 1293, 2586]
	arrays, _ = R.chain_graph_arrays(n_edges)
	pairs, n_bins = R.trials_at(R.state_at(bits, cand_edge[2590])[1], cand_edge, [int(a) for a in arrays["aligned_positions"]], 2590, 0, n_edges)
	assert 4 == n_bins and pairs == [(2586, 1), (1293, 2), (2, 3), (1, 4), (0, 5)]


def test_minimum_distance_equal_to_a_candidate_distance():
	"""min_distance == the distance to a candidate that is tried keeps its pair, one more drops it (find_cut_positions.cc:151: <=)."""
	n = 30
	arrays, _ = R.chain_graph_arrays(n, seed=1)
	cand_edge, _, cand_aligned = R.every_node_candidates(n, arrays["aligned_positions"])
	div = R.state_at(R.family("identity", n, n), cand_edge[20])[1]
	distance = cand_aligned[20] - cand_aligned[12]
	with_it, _ = R.trials_at(div, cand_edge, cand_aligned, 20, distance, n)
	without, _ = R.trials_at(div, cand_edge, cand_aligned, 20, distance + 1, n)
	assert 12 in [p for p, _ in with_it] and 12 not in [p for p, _ in without[:-1]] and len(without) < len(with_it)
	# larger than the whole alignment: only the final pair is left
	# (the identity family's values reach down to the sentinel, so no final pair follows them; dense bits leave one)
	assert R.trials_at(div, cand_edge, cand_aligned, 20, cand_aligned[-1] + 1, n)[0] == []
	div = R.state_at(R.family("dense", n, n), cand_edge[20])[1]
	everything, _ = R.trials_at(div, cand_edge, cand_aligned, 20, 0, n)
	final = [p for p in everything if p[1] == n]                                # (the loop's pairs count fewer than all copies)
	assert 1 == len(final) and len(everything) > 1 and R.trials_at(div, cand_edge, cand_aligned, 20, cand_aligned[-1] + 1, n)[0] == final
