// Bootstrap support of a neighbour-joining tree (include/v2m_hip.h, "bootstrap"): how many replicate trees hold the split of each
// join record of the main tree.  Plain C++, no HIP: v2m_hip.hip includes it for v2m_nj_bootstrap and the host library exports it as
// v2mh_nj_split_support.
//
// The split of join record t is the set of leaves under node n + t against the rest; as a bit set over the leaves it is normalised
// to the side WITHOUT leaf 0, so that a split is one value whichever side a tree's node lies on.  The records come in order of
// creation (a child is made before it is joined), so the sets are built bottom-up in one pass, without recursion: (n - 3) sets of
// ceil(n / 64) words a tree.  The main tree's sets are indexed by a hash of their words; a replicate's set counts for record t only
// where its words EQUAL those of t: the hash picks the candidates and never decides.
#pragma once

#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/v2m_hip.h"

namespace v2m {

// Empty when the n - 2 records are a tree over n >= 3 leaves -- every id but the root's is a child exactly once, a node is made before
// it is joined, and only the last record has a third child --, else what is wrong.
inline std::string nj_records_error(v2m_nj_node const *nodes, std::uint64_t n)
{
	if (n < 3) return "a tree has at least 3 leaves";
	std::uint64_t const root(n - 3);
	std::vector<char> used(2 * n - 3, 0);
	for (std::uint64_t rec(0); rec <= root; ++rec) {
		v2m_nj_node const &nd(nodes[rec]);
		if ((rec < root) != (V2M_NJ_NONE == nd.c))
			return "record " + std::to_string(rec) + " of the tree has " + (rec < root ? "three children" : "two children, and is the last");
		for (int k(0); k < (rec < root ? 2 : 3); ++k) {
			std::uint64_t const child(0 == k ? nd.a : 1 == k ? nd.b : nd.c);
			if (child >= n + rec) return "record " + std::to_string(rec) + " of the tree names node " + std::to_string(child) + ", which is not made before it";
			if (used[child]) return "node " + std::to_string(child) + " of the tree is joined twice";
			used[child] = 1;
		}
	}
	return std::string();
}

// The normalised splits of the join records 0 ... n - 4 of a checked tree: sets[t * words + w], words = ceil(n / 64).
inline void nj_split_sets(v2m_nj_node const *nodes, std::uint64_t n, std::vector<std::uint64_t> &sets)
{
	std::uint64_t const words((n + 63) / 64), joins(n - 3);
	sets.assign(joins * words, 0);
	std::vector<char> complemented(joins, 0);   // the stored set is the leaves NOT under the node
	for (std::uint64_t t(0); t < joins; ++t) {
		std::uint64_t *const set(&sets[t * words]);
		for (int k(0); k < 2; ++k) {
			std::uint64_t const child(0 == k ? nodes[t].a : nodes[t].b);
			if (child < n) set[child / 64] |= std::uint64_t(1) << (child % 64);
			else {
				std::uint64_t const *const below(&sets[(child - n) * words]);
				bool const flipped(complemented[child - n]);
				for (std::uint64_t w(0); w < words; ++w) set[w] |= flipped ? ~below[w] : below[w];
			}
		}
		if (n % 64) set[words - 1] &= (std::uint64_t(1) << (n % 64)) - 1;
		if (set[0] & 1) {
			complemented[t] = 1;
			for (std::uint64_t w(0); w < words; ++w) set[w] = ~set[w];
			if (n % 64) set[words - 1] &= (std::uint64_t(1) << (n % 64)) - 1;
		}
	}
}

inline std::uint64_t nj_split_hash(std::uint64_t const *set, std::uint64_t words)
{
	std::uint64_t h(0x9E3779B97F4A7C15ULL);
	for (std::uint64_t w(0); w < words; ++w) {
		h ^= set[w];
		h ^= h >> 30; h *= 0xBF58476D1CE4E5B9ULL;
		h ^= h >> 27; h *= 0x94D049BB133111EBULL;
		h ^= h >> 31;
	}
	return h;
}

// Counts, for the join records of one main tree, the trees that hold their splits: begin() once, add() per tree.  Both return the
// empty string, or what is wrong with a tree that is none.
class nj_split_counter {
public:
	// support: n - 3 counts, zeroed here (nothing with n == 3)
	std::string begin(std::uint64_t n, v2m_nj_node const *main_nodes, std::uint32_t *support)
	{
		std::string const err(nj_records_error(main_nodes, n));
		if (!err.empty()) return err;
		m_n = n; m_words = (n + 63) / 64; m_support = support;
		nj_split_sets(main_nodes, n, m_main);
		m_by_hash.clear();
		m_by_hash.reserve(n - 3);
		for (std::uint64_t t(0); t < n - 3; ++t) {
			m_by_hash.emplace(nj_split_hash(&m_main[t * m_words], m_words), t);
			support[t] = 0;
		}
		return std::string();
	}

	std::string add(v2m_nj_node const *nodes)
	{
		std::string const err(nj_records_error(nodes, m_n));
		if (!err.empty()) return err;
		nj_split_sets(nodes, m_n, m_sets);
		for (std::uint64_t t(0); t < m_n - 3; ++t) {
			std::uint64_t const *const set(&m_sets[t * m_words]);
			auto const range(m_by_hash.equal_range(nj_split_hash(set, m_words)));
			for (auto it(range.first); it != range.second; ++it) {   // (the hash picks, the words decide)
				if (0 == std::memcmp(set, &m_main[it->second * m_words], m_words * sizeof(std::uint64_t))) { ++m_support[it->second]; break; }
			}
		}
		return std::string();
	}

private:
	std::uint64_t m_n{}, m_words{};
	std::uint32_t *m_support{};
	std::vector<std::uint64_t> m_main, m_sets;
	std::unordered_multimap<std::uint64_t, std::uint64_t> m_by_hash;
};

// support[t], t = 0 ... n - 4: the replicates (n_replicates trees of n - 2 records each, one after the other) that hold the split of
// record t of the main tree.  Returns the empty string, or what is wrong with the first tree that is none (support is then
// unspecified).  With n == 3 nothing is written.
inline std::string nj_split_support(std::uint64_t n, v2m_nj_node const *main_nodes, v2m_nj_node const *replicate_nodes, std::uint64_t n_replicates, std::uint32_t *support)
{
	nj_split_counter counter;
	{
		std::string const err(counter.begin(n, main_nodes, support));
		if (!err.empty()) return "the main tree: " + err;
	}
	for (std::uint64_t r(0); r < n_replicates; ++r) {
		std::string const err(counter.add(replicate_nodes + r * (n - 2)));
		if (!err.empty()) return "replicate " + std::to_string(r) + ": " + err;
	}
	return std::string();
}

} // namespace v2m
