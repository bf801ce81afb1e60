// output.hh -- the output classes of the reference (include/vcf2multialign/output.hh:26-130) over the GPU path.
//
// Same class names, constructor arguments and row/identifier conventions; output_a2m() batches all rows of a
// file into one v2m_splice_rows() call instead of calling output_sequence() per row.  With pipe_cmd the sequences go
// to the standard input of `pipe_cmd <name>` instead of a file (output.cc:26-38,49-68).
// founder_sequence_greedy_output takes its cut positions and matchings from founder.hh (find_cut_positions /
// find_matchings, sequential host algorithms) or from a cut-position file.
#pragma once

#include <cstdint>
#include <functional>
#include <ostream>
#include <string>
#include <utility>
#include <vector>

#include "gpu_path.hh"

namespace v2m::host {

struct output_delegate {
	virtual ~output_delegate() {}
	virtual void will_handle_sample(std::string const &sample, u32 sample_idx, u32 chr_copy_idx) = 0;
	virtual void will_handle_founder_sequence(u32 idx) = 0;
	virtual void handled_sequences(u32 sequence_count) = 0;
};

struct null_output_delegate final : output_delegate {
	void will_handle_sample(std::string const &, u32, u32) override {}
	void will_handle_founder_sequence(u32) override {}
	void handled_sequences(u32) override {}
};

// One region of --regions-file: alignment columns [col_begin, col_end) go to the file `name` + ".a2m" (".fa" unaligned).
struct output_region {
	std::string name;
	u64 col_begin{}, col_end{};
};

// One UCSC chain (reference -> row) from a row's alignment ops (include/v2m_hip.h, "row alignment ops"): a pure function of its arguments.
//   chain <score> <t_name> <t_size> + <tStart> <tEnd> <q_name> <q_size> + <qStart> <qEnd> <id>
//   <size> <dt> <dq>      one line per M op but the last: dt / dq are the summed D / I lengths between it and the next M op
//   <size>                the last M op
//   (a blank line)
// score = the summed M lengths; leading and trailing I / D ops move tStart / qStart and tEnd / qEnd inward from 0 and the sizes.
// Ops without any M give the empty string (no chain).  Throws std::invalid_argument for an op code other than M, I, D.
std::string chain_text(v2m_aln_op const *ops, u64 n_ops, std::string const &t_name, u64 t_size, std::string const &q_name, u64 q_size, u64 id);

// One PAF line (the row as query, the reference as target) from a row's SPLIT alignment ops (V2M_OPS_SPLIT_MATCH: =, X, I, D), as
// minimap2 --eqx -c writes it: a pure function of its arguments.  Tab-separated, ending in '\n':
//   q_name q_size qStart qEnd + t_name t_size tStart tEnd n_eq block_len 255 NM:i:<n> cg:Z:<cigar>
// Leading and trailing I / D ops move qStart / tStart and qEnd / tEnd inward, as in chain_text; the cigar is the ops from the first to
// the last = / X op inclusive, each <length><=|X|I|D>; n_eq = the summed = lengths, block_len = the summed lengths of the cigar's ops,
// NM = block_len - n_eq.  Ops without any = / X give the empty string (no line).  Throws std::invalid_argument for an op code other
// than =, X, I, D: a caller that passes M has not asked for the split.
std::string paf_text(v2m_aln_op const *ops, u64 n_ops, std::string const &t_name, u64 t_size, std::string const &q_name, u64 q_size);

// Split ops folded back to those of flags = 0: = and X become M, equal neighbours merge.
std::vector<v2m_aln_op> fold_split_ops(v2m_aln_op const *ops, u64 n_ops);

// The TSV of column counts (include/v2m_hip.h, "column counts"): a pure function of its arguments.
//   #rows<TAB><n_rows>
//   #column<TAB>ref_pos<TAB>A<TAB>C<TAB>G<TAB>T<TAB>N<TAB>gap<TAB>other
//   one line per record: the 0-based aligned column; the 1-based reference position whose byte the REF row holds there -- with n the
//   last node with aligned_positions[n] <= column and k = column - aligned_positions[n]: reference_positions[n] + k + 1 when
//   k < reference_positions[n + 1] - reference_positions[n], else `.` (the REF row has padding there) --; the six counts; other =
//   n_rows minus their sum.
std::string column_counts_text(u64 n_rows, v2m_column_count const *records, u64 n_records, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count);

// The TSV of pair distances (include/v2m_hip.h, "pair distances"), as snp-dists writes its matrix: a pure function of its arguments.
//   #rows<TAB><n><TAB>columns<TAB><n_columns><TAB>sites<TAB><n_sites><TAB>model<TAB>all|acgt
//   id<TAB><ids[0]><TAB>...<TAB><ids[n - 1]>
//   one line per sequence: its id, then its n distances (dist is n x n, row-major)
// An id that holds a tab or a line break is refused.
std::string distances_text(std::vector<std::string> const &ids, std::uint32_t const *dist, u64 n_columns, u64 n_sites, bool acgt_only);

// The --output-site-positions file of the variable sites (include/v2m_hip.h, "variable sites"): one line per site,
//   <column><TAB><reference position | .>
// the first two fields of that column's line of column_counts_text, made by the same code.
std::string site_positions_text(u64 const *columns, u64 n_sites, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count);

// --output-ld's text: a `#rows` line with the figures of the call and its parameters, a header line, then per pair the column and the
// reference position of both sites (the first two fields of their --output-column-counts lines), n, n_a, n_b, n_ab and r2 =
// (double) D^2 / (double) den with D^2 and den as 64-bit integers, printed %.6f.  Throws when a pair names a site beyond n_sites or has
// den = 0 (the library reports no such pair).
std::string site_ld_text(u64 n_rows, u64 n_columns, v2m_ld_site const *sites, u64 n_sites, v2m_ld_pair const *pairs, u64 n_pairs, v2m_site_ld_params const &params,
	u64 const *reference_positions, u64 const *aligned_positions, u64 node_count);

// --ld-min-r2's value from its digits, with no floating point: DIGITS[.DIGITS], at most 6 decimals, inside [0, 1]; in lowest terms.
bool parse_decimal_fraction(char const *text, std::uint32_t &numerator, std::uint32_t &denominator);

// The neighbour-joining tree (include/v2m_hip.h, "neighbour joining") of the n >= 3 taxa of dist (u32[n][pitch], of which only the
// upper triangle is read), restated in plain loops: nodes receives the n - 2 records.  The second yardstick of the GPU's result and
// the CPU baseline of its measurement.  O(n^3) time, n^2 doubles of memory.
void nj_tree_cpu(std::uint32_t const *dist, u64 n, u64 pitch, v2m_nj_node *nodes);

// --output-tree's text: the tree of the n - 2 records over the n leaves named `labels` in Newick form, a pure function of its
// arguments.  Node n + t is written (<a>:<len_a>,<b>:<len_b>), the tree (<a>:...,<b>:...,<c>:...); and a line break; internal nodes
// carry no label; lengths are printed %.10g.  A label of A-Z, a-z, 0-9, '.' and '-' only is written bare, any other (an empty one and
// one with '_', which a Newick reader would take for a space, included) in single quotes with ' doubled.  Built without recursion.
// Throws when the records are no tree over the leaves: an id out of range or used twice, or c set before the last record.
std::string nj_newick_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels);

// nj_newick_text with the support of every join node as its label: node n + t is written (<a>:<len_a>,<b>:<len_b>)<support[t]>, the
// count in decimal.  support holds n - 3 counts (none is read with 3 leaves); the trifurcation carries no label.
std::string nj_newick_support_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels, std::uint32_t const *support);

// v2m::nj_split_support of csrc/nj_support.hpp, throwing what it reports.
void nj_split_support(u64 n_leaves, v2m_nj_node const *main_nodes, v2m_nj_node const *replicate_nodes, u64 n_replicates, std::uint32_t *support);

// Parsimony on a tree (include/v2m_hip.h, "parsimony") restated in plain loops over bytes (u8[n][pitch], of which the first n_sites
// bytes of a row count) and the n - 2 records: sites receives n_sites records, branch_changes 2 n - 3 counts, and mutations -- which
// may be NULL with capacity 0 -- the list when it fits capacity.  Returns the number of mutations.  The yardstick of the GPU's result
// and the CPU baseline of its measurement.  Throws std::invalid_argument when the records are no tree in the header's sense.
u64 tree_parsimony_cpu(unsigned char const *bytes, u64 n, u64 n_sites, u64 pitch, v2m_nj_node const *nodes, v2m_parsimony_site *sites, std::uint32_t *branch_changes,
	v2m_tree_mutation *mutations, u64 capacity);

// --output-tree-parsimony's text: the topology nj_newick_text writes, every branch length the integer branch_changes[x] of the
// branch's lower node x, every internal node labelled node<t> by its record, the root included: (...)node7:3 and (...)node<n - 3>;
std::string nj_newick_parsimony_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels, std::uint32_t const *branch_changes);

// --output-tree-mutations' text: one line per mutation, in the list's order,
//   <node><TAB><column><TAB><reference position | .><TAB><from><TAB><to>
// node the leaf's label or node<t>, column and position as site_positions_text writes them for the mutation's site, from and to of ACGT.
std::string tree_mutations_text(v2m_tree_mutation const *mutations, u64 n_mutations, v2m_tree_site const *sites, u64 n_sites, std::vector<std::string> const &labels,
	u64 const *reference_positions, u64 const *aligned_positions, u64 node_count);

// --output-tree-sites' text: one line per site,
//   <column><TAB><reference position | .><TAB><states><TAB><steps><TAB><homoplasy>
// states the letters of ACGT present, homoplasy = steps - (popcount(present) - 1) as a signed number.
std::string tree_sites_text(v2m_tree_site const *sites, u64 n_sites, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count);

// Window diversity (include/v2m_hip.h, "window diversity") restated in plain loops from spliced rows, not from a counts table: rows_a is
// u8[n_a][pitch] and, for the between form, rows_b u8[n_b][pitch] (else NULL), of which the first L bytes of a row count; bounds are
// relative to the rows, bounds[n_bins] <= L.  Per column the letters of every row are tallied; diffs is (m^2 - the sum of the squared
// tallies) / 2 within and the sum over unlike letters of the two groups' tallies between -- neither is the expression the kernel uses.
// bins receives n_bins records of v2m_diversity_bin (within) or v2m_diversity_between_bin (between); sfs (within only, may be NULL)
// n_a / 2 + 1 entries; *multiallelic (may be NULL) the count the spectrum defines.  Throws std::invalid_argument for descending bounds,
// bounds beyond L or the pitch, or a spectrum in the between form.
void window_diversity_cpu(unsigned char const *rows_a, u64 n_a, unsigned char const *rows_b, u64 n_b, u64 L, u64 pitch, u64 const *bounds, u64 n_bins, void *bins, u64 *sfs,
	u64 *multiallelic);

// The doubles of the header, operation by operation; a value that does not exist is a quiet NaN.
struct diversity_values { double pi, theta_w, tajima_d; };
diversity_values diversity_values_of(v2m_diversity_bin const &window, u64 n);
struct divergence_values { double dxy, fst; };
divergence_values divergence_values_of(v2m_diversity_between_bin const &between, v2m_diversity_bin const &window_a, v2m_diversity_bin const &window_b);

// --output-diversity's lines for one group of n sequences: one per window,
//   <group><TAB><start><TAB><end><TAB>columns<TAB>called<TAB>diffs<TAB>pairs<TAB>pi<TAB>segregating<TAB>complete<TAB>theta_w<TAB>tajima_d
// start and end as given (the driver passes 1-based inclusive reference positions), the integers of the window's record (segregating
// and complete are its counts over all and over complete columns), the doubles printed %.10g as the Newick writer prints lengths, NA
// where a value does not exist.  header: the line of column names, beginning with '#', first.
std::string window_diversity_text(std::string const &group, u64 n, v2m_diversity_bin const *windows, u64 const *starts, u64 const *ends, u64 n_windows, bool header);

// --output-divergence's lines for one pair of groups:
//   <group_a><TAB><group_b><TAB><start><TAB><end><TAB>columns<TAB>called<TAB>diffs<TAB>pairs<TAB>dxy<TAB>fst
std::string window_divergence_text(std::string const &group_a, std::string const &group_b, v2m_diversity_between_bin const *between, v2m_diversity_bin const *windows_a,
	v2m_diversity_bin const *windows_b, u64 const *starts, u64 const *ends, u64 n_windows, bool header);

// --diversity-sfs' lines for one group: <group><TAB><n><TAB><minor count><TAB><columns> for every entry of the folded spectrum, then
// <group><TAB><n><TAB>multiallelic<TAB><count>.
std::string diversity_sfs_text(std::string const &group, u64 n, u64 const *sfs, u64 multiallelic, bool header);

class output {
public:
	output(gpu_context &gpu, char const *pipe_cmd, char const *chromosome_id, bool should_output_reference, bool should_output_unaligned, output_delegate &delegate);
	virtual ~output() {}

	// The graph must be the one uploaded to the context (upload_graph()).
	virtual void output_separate(variant_graph const &graph, bool should_include_fasta_header) = 0;
	void output_a2m(variant_graph const &graph, char const *dst_name);

	// More GPUs for the same output (each must hold the same uploaded graph): the rows of an aligned A2M file are
	// then sharded in contiguous blocks over all contexts, one host thread per context, and every thread writes its
	// rows straight to their final place in the file (every aligned row has the same length, so offsets are known
	// up front; there is no collective and no reordering buffer -- SURVEY.md section 8e).  Unaligned output and
	// std::ostream targets use the first context only.
	void add_gpu(gpu_context &gpu) { m_more_gpus.push_back(&gpu); }

	// The chromosome copies each context's path matrix holds (one entry per context, the first context first), when the
	// matrix was sharded with upload_path_slice(): rows of a plain haplotype batch then go to the context that owns their
	// copy, with the copy index re-based to the shard (the REF row to the first context).  Without shards every context is
	// expected to hold the whole matrix and rows are split evenly.
	void set_copy_shards(std::vector<copy_shard> shards) { m_copy_shards = std::move(shards); }

	// The other way to share the path matrix, for every output that has to leave in row order (std::ostream targets: pipes,
	// unaligned A2M; one file per sequence): the contexts hold the chromosome copies dealt round-robin in blocks
	// (upload_path_blocks()), every context splices ITS rows on its own thread, and the rows are handed to the one writer in
	// row order straight from the contexts' pinned buffers (no copy, no queue: a turnstile on the row index).  While one
	// context's rows are being written, the others' next blocks are crossing PCIe.
	void set_copy_interleave(copy_interleave deal) { m_copy_interleave = deal; m_interleaved = true; }

	// A2M output as BGZF (include/v2m_hip.h, "BGZF output"; the --bgzf extension): the rows' bodies compressed on the GPU
	// (V2M_SPLICE_BGZF), the text around them in stored members, an EOF member at the end.  Decompressed, the file is the plain A2M.
	// Only output_a2m() uses it; with several contexts the rows take the interleaved path (set_copy_interleave()), never the sharded
	// one, whose file offsets are known up front.
	void set_bgzf(bool bgzf) { m_bgzf = bgzf; }

	// --regions-file: one file per region in the working directory, each holding every row of the A2M output (same order, same
	// identifiers) cut to the region's columns -- byte for byte what output_a2m() writes under that region's column window.  The
	// regions of a pass are one window set (include/v2m_hip.h, "window sets") spliced in one call; a pass holds at most
	// regions_per_pass regions (as many files are open at once), more regions take more passes.  First context only.
	// distinct (--distinct): a region's file holds one record per distinct body, in the order of first occurrence -- the plain file
	// without every record whose body occurred earlier in it --, and `name` + ".classes.tsv" one line per row: its identifier, the
	// identifier of the first row with the same body, and that body's index in the file.  The duplicates are found on the device
	// (v2m_splice_window_set_distinct) and only the distinct bodies come to the host; verbose prints per pass the pieces, the distinct
	// pieces and the bytes that crossed the link to stderr.
	void output_regions(variant_graph const &graph, std::vector<output_region> const &regions, std::size_t regions_per_pass, bool distinct = false, bool verbose = false);
	virtual void output_a2m(variant_graph const &graph, std::ostream &stream) = 0;

	// --output-chain: one chain per output row (chain_text above: the reference as target, the row as query) into `path`, from
	// v2m_row_ops on the first context, which must hold every copy.  Rows and order are those of the A2M output minus the REF row
	// (which has no chain, whatever should_output_reference says); tName is prefixed("REF", '.'), qName the row's name as
	// output_separate() forms it without a suffix, id the 1-based number of the chain's row.  A name with whitespace in it is a
	// std::runtime_error before any GPU work; a row without any M op gets no chain and a warning on stderr.
	void output_chain(variant_graph const &graph, char const *path);
	void output_chain(variant_graph const &graph, std::ostream &stream);

	// --output-paf: one PAF line per output row (paf_text above) from v2m_row_ops with V2M_OPS_SPLIT_MATCH; the rows, their names and
	// the whitespace check are output_chain's.  The REF row has no line; a row without any = / X op gets none and a warning on stderr.
	void output_paf(variant_graph const &graph, char const *path);
	void output_paf(variant_graph const &graph, std::ostream &stream);
	// Both files from ONE pass over the rows, with the split: the chains are made from the ops folded back (fold_split_ops) and are
	// byte for byte those of output_chain().
	void output_chain_and_paf(variant_graph const &graph, char const *chain_path, char const *paf_path);
	void output_chain_and_paf(variant_graph const &graph, std::ostream &chain_stream, std::ostream &paf_stream);

	// --output-column-counts: column_counts_text above for the rows of the A2M output (REF first, unless omitted) over the view in force
	// (--region: the window's columns, reported as absolute), from v2m_column_counts on the first context, which must hold every
	// copy.  Variable columns only unless all_columns; verbose prints the rows, columns and variable columns to stderr.
	void output_column_counts(variant_graph const &graph, char const *path, bool all_columns = false, bool verbose = false);
	void output_column_counts(variant_graph const &graph, std::ostream &stream, bool all_columns = false, bool verbose = false);

	// --output-distances: distances_text above for the rows of the A2M output (REF first, unless omitted) under the names --output-paf
	// writes, over the view in force (--region: the window's columns), from v2m_pair_distances on the first context, which must hold
	// every copy.  acgt_only: V2M_DIST_ACGT_ONLY; verbose prints the rows, columns, sites and passes to stderr.
	void output_distances(variant_graph const &graph, char const *path, bool acgt_only = false, bool verbose = false);
	void output_distances(variant_graph const &graph, std::ostream &stream, bool acgt_only = false, bool verbose = false);

	// --output-variable-sites: a FASTA file of the rows of the A2M output (REF first, unless omitted) under the names the -s file gives
	// them, every sequence line cut down to the selected columns of the view in force (--region: the window's columns): the -s file
	// with only its variable columns, from v2m_variable_sites on the first context, which must hold every copy.  snp_only:
	// V2M_SITES_SNP; positions: site_positions_text above goes there; verbose prints the rows, columns and sites to stderr.
	void output_variable_sites(variant_graph const &graph, char const *path, bool snp_only = false, char const *positions_path = nullptr, bool verbose = false);
	void output_variable_sites(variant_graph const &graph, std::ostream &stream, bool snp_only = false, std::ostream *positions = nullptr, bool verbose = false);

	// --output-ld: site_ld_text above for the rows of the A2M output (REF first, unless omitted), from v2m_site_ld on the first context,
	// which must hold every copy.  The reported pairs are kept (24 bytes each) until the last has arrived: the first line holds their
	// number.  verbose prints the rows, columns, sites, candidates and pairs to stderr.
	void output_ld(variant_graph const &graph, char const *path, v2m_site_ld_params const &params, bool verbose = false);
	void output_ld(variant_graph const &graph, std::ostream &stream, v2m_site_ld_params const &params, bool verbose = false);

	// --output-tree: nj_newick_text above for the rows of the A2M output (REF first, unless omitted) under the names --output-distances
	// writes, over the view in force (--region: the window's columns), from v2m_nj_tree on the first context, which must hold every
	// copy.  acgt_only: V2M_DIST_ACGT_ONLY; verbose prints the rows, columns, sites and joins to stderr.
	// bootstrap > 0 (--tree-bootstrap, with seed: --tree-seed): the tree and the support of its joins from v2m_nj_bootstrap, written by
	// nj_newick_support_text; replicates (--output-tree-replicates), when given, receives the replicate trees, a line of
	// nj_newick_text each.  verbose then prints the replicates, the largest K and the pack passes as well.
	void output_tree(variant_graph const &graph, char const *path, bool acgt_only = false, bool verbose = false,
		std::uint32_t bootstrap = 0, std::uint64_t seed = 1, char const *replicates_path = nullptr);
	void output_tree(variant_graph const &graph, std::ostream &stream, bool acgt_only = false, bool verbose = false,
		std::uint32_t bootstrap = 0, std::uint64_t seed = 1, std::ostream *replicates = nullptr);

	// --output-tree-parsimony, --output-tree-mutations, --output-tree-sites: nj_newick_parsimony_text, tree_mutations_text and
	// tree_sites_text above (each where its stream or path is given) from v2m_tree_parsimony on the tree the last output_tree() call of
	// this object wrote -- with a bootstrap, the main tree --, for the same rows under the same names and over the view in force.  The
	// mutations are kept (16 bytes each) until the last has arrived.  verbose prints the rows, columns, sites, mutations and ranges.
	void output_tree_parsimony(variant_graph const &graph, char const *newick_path, char const *mutations_path, char const *sites_path, bool verbose = false);
	void output_tree_parsimony(variant_graph const &graph, std::ostream *newick, std::ostream *mutations, std::ostream *sites, bool verbose = false);

	// --output-diversity, --diversity-sfs, --output-divergence: window_diversity_text, diversity_sfs_text and window_divergence_text
	// above (each where its stream or path is given) for the rows of the A2M output under the names --output-distances writes, over
	// the 0-based half-open reference range [ref_begin, ref_end) -- the view in force must be its columns (--region), or whole rows
	// -- from the first context, which must hold every copy.  The range is cut into bins of `step` positions, the last one perhaps
	// shorter; bin k begins at the column of position ref_begin + k * step (columns_of_reference_range), so the columns of an
	// insertion fall to the bin of the reference position before them.  Window j is the bins [j, j + window / step) summed field by
	// field, for every j with a whole window, or the one short window where the range holds none; start and end are its first and
	// last reference position, 1-based.  groups: (sequence id, group name) pairs; a sequence not named belongs to no group, an id that
	// names no row throws, and so do more than 16 groups; empty: one group, `all`, of every row (v2m_window_diversity).  With groups
	// every group is counted once into a table of v2m_alloc_output (v2m_column_counts_device) and v2m_diversity_of_counts runs per
	// group and per pair; the tables together may take V2M_DIVERSITY_TABLE_BYTES (environment, read per call; default 16 GiB) at
	// most, more throws with the figure.  divergence needs at least two groups.
	struct diversity_params {
		u64 window{10000}, step{10000};
		u64 ref_begin{}, ref_end{}, ref_len{};
		std::vector<std::pair<std::string, std::string>> groups;
	};
	void output_diversity(variant_graph const &graph, diversity_params const &params, char const *diversity_path, char const *sfs_path, char const *divergence_path, bool verbose = false);
	void output_diversity(variant_graph const &graph, diversity_params const &params, std::ostream *diversity, std::ostream *sfs, std::ostream *divergence, bool verbose = false);
	// the ids output_diversity names the rows by (what a --diversity-groups file may hold)
	std::vector<std::string> diversity_ids(variant_graph const &graph) { return chain_rows(graph).ids; }

protected:
	struct row_set {
		std::vector<std::string> ids;           // FASTA identifiers (a2m) or file names (separate)
		std::vector<std::uint32_t> copy_index;
		std::vector<std::uint64_t> cut_offsets{0}, cut_nodes;
		std::vector<std::uint32_t> cut_copies;
		bool any_cuts{};
	};
	// the sink sees the rows in batch order, one at a time; extra_flags: V2M_SPLICE_BGZF or 0
	void splice(row_set const &rows, v2m_sink_fn sink, void *user, std::uint32_t extra_flags = 0);
	void splice_in_turns(row_set const &rows, v2m_sink_fn sink, void *user, std::uint32_t extra_flags = 0);
	// rows that need no order and a sink that keeps them until it calls v2m_row_release (a pool of writers): v2m_splice_rows_held per context
	void splice_held(row_set const &rows, v2m_hold_sink_fn sink, void *user);
	static std::vector<std::uint32_t> rebased_copies(row_set const &rows, std::uint64_t first, std::uint64_t last, copy_shard shard);
	void write_a2m(row_set const &rows, std::ostream &stream);
	void write_a2m_sharded(row_set const &rows, char const *dst_name);
	virtual row_set a2m_rows(variant_graph const &graph) = 0;
	// `open_chain` / `open_paf` (either may be empty, not both) are called once the names are checked; with open_paf the rows go through v2m_row_ops with the split
	void write_chains(variant_graph const &graph, std::function<std::ostream &()> const &open_chain, std::function<std::ostream &()> const &open_paf = {});
	virtual row_set chain_rows(variant_graph const &graph) = 0;   // the rows of a2m_rows() under the names of output_separate()
	void write_separate(row_set const &rows);
	std::string prefixed(std::string const &name, char sep) const;

	gpu_context &m_gpu;
	std::vector<gpu_context *> m_more_gpus;
	std::vector<copy_shard> m_copy_shards;
	copy_interleave m_copy_interleave;
	bool m_interleaved{};
	char const *m_pipe_cmd{};
	char const *m_chromosome_id{};
	output_delegate *m_delegate{};
	bool m_should_output_reference{};
	bool m_should_output_unaligned{};
	bool m_bgzf{};
	std::vector<v2m_nj_node> m_tree_nodes;   // the main tree of the last output_tree()
};

class haplotype_output final : public output {
public:
	using output::output;
	using output::output_a2m;
	void output_separate(variant_graph const &graph, bool should_include_fasta_header) override;
	void output_a2m(variant_graph const &graph, std::ostream &stream) override;
private:
	row_set rows_for(variant_graph const &graph, char sep, char const *suffix);
	row_set a2m_rows(variant_graph const &graph) override { return rows_for(graph, '\t', ""); }
	row_set chain_rows(variant_graph const &graph) override { return rows_for(graph, '.', ""); }
};

class founder_sequence_greedy_output final : public output {
public:
	using output::output;
	using output::output_a2m;
	// cut_positions: node indices, first 0, last the sink; assigned_samples: (cuts - 1) rows x founders columns,
	// column-major, one column per founder (founder_sequence_greedy_output.cc:171,544).
	void set_cut_positions(std::vector<u64> cut_positions) { m_cut_positions = std::move(cut_positions); }
	void set_assigned_samples(std::vector<u32> column_major, u32 founder_count) { m_assigned_samples = std::move(column_major); m_founder_count = founder_count; }
	void output_separate(variant_graph const &graph, bool should_include_fasta_header) override;
	void output_a2m(variant_graph const &graph, std::ostream &stream) override;
private:
	row_set rows_for(char sep, char const *suffix);
	row_set a2m_rows(variant_graph const &) override { return rows_for('\t', ""); }
	row_set chain_rows(variant_graph const &) override { return rows_for('.', ""); }
	std::vector<u64> m_cut_positions;
	std::vector<u32> m_assigned_samples;
	u32 m_founder_count{};
};

} // namespace v2m::host
