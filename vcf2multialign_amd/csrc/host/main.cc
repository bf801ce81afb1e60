// main.cc -- thin command-line driver with the reference's flag names (vcf2multialign/cmdline.ggo:4-55,
// vcf2multialign/main.cc:370-552) for the part this repository implements: --haplotypes and --founder-sequences with
// FASTA + VCF (or checkpointed graph) input, A2M / separate / unaligned / piped output, sample filters, overlap
// reports, cut-position files.  The per-row splicing and the path-matrix
// transpose run on the GPU (there is no CPU path); everything else is host code.

#include <getopt.h>
#include <sys/resource.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <map>
#include <thread>
#include <iostream>
#include <memory>
#include <set>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include <chrono>
#include <csignal>

#include "founder.hh"
#include "gpu_path.hh"
#include "graph_file.hh"
#include "output.hh"
#include "readers.hh"

namespace vh = v2m::host;

namespace {

struct options {
	bool haplotypes{};
	long founder_sequences{0};
	long minimum_distance{0};
	bool founder_mode{}, keep_ref_edges{};
	char const *input_reference{}, *reference_sequence{}, *input_variants{}, *chromosome{};
	char const *output_sequences_a2m{}, *dst_chromosome{}, *output_overlaps{};
	char const *include_samples{}, *exclude_samples{};
	char const *input_graph{}, *output_graph{};
	char const *pipe{}, *input_cut_positions{}, *output_cut_positions{};
	bool output_sequences_separate{}, separate_plain{}, omit_reference{}, unaligned{}, verbose{}, graph_statistics{};
	bool ref_mismatch_error{};
	bool bgzf{};
	bool gpu_parse{};                     // --gpu-parse: the genotype columns of -a become path bits on the GPU (v2m_vcf_scan)
	char const *region{};                 // --region=START-END: 1-based inclusive positions on the reference sequence
	std::uint64_t region_start{}, region_end{};
	char const *output_chain{};           // --output-chain=FILE: one UCSC chain per output row (reference -> row), from v2m_row_ops
	char const *output_paf{};             // --output-paf=FILE: one PAF line with an =/X/I/D cigar per output row, from v2m_row_ops with V2M_OPS_SPLIT_MATCH
	char const *regions_file{};           // --regions-file=FILE.bed: one output file per BED region, all spliced as one window set per pass
	char const *output_column_counts{};   // --output-column-counts=FILE: base counts per variable alignment column, from v2m_column_counts
	char const *output_distances{};       // --output-distances=FILE: the matrix of pairwise distances between the output rows, from v2m_pair_distances
	bool acgt_only{};                     // --acgt-only (with --output-distances): only columns where both rows hold A, C, G or T count
	char const *output_variable_sites{};  // --output-variable-sites=FILE: the output rows cut down to the variable columns, as FASTA, from v2m_variable_sites
	char const *output_site_positions{};  // --output-site-positions=FILE (with --output-variable-sites): the column and the reference position of every site
	bool snp_sites{};                     // --snp-sites (with --output-variable-sites): only columns where at least two of A, C, G, T occur
	char const *output_ld{};              // --output-ld=FILE: linkage disequilibrium between nearby biallelic sites of the output rows, from v2m_site_ld
	char const *ld_window{}, *ld_window_columns{}, *ld_min_r2{}, *ld_min_count{};   // --ld-window=SITES, --ld-window-columns=N, --ld-min-r2=DECIMAL, --ld-min-count=N (with --output-ld)
	v2m_site_ld_params ld_params{1000, 1, 1, 5, 0};
	char const *output_tree{};            // --output-tree=FILE: the neighbour-joining tree of the output rows in Newick form, from v2m_nj_tree
	bool tree_acgt_only{};                // --tree-acgt-only (with --output-tree): the tree of the distances --acgt-only counts
	char const *tree_bootstrap{}, *tree_seed{};   // --tree-bootstrap=B (with --output-tree), --tree-seed=S (with --tree-bootstrap; default 1)
	char const *output_tree_replicates{};         // --output-tree-replicates=FILE (with --tree-bootstrap): the replicate trees, a Newick line each
	std::uint32_t tree_replicates{};              // B, or 0: no bootstrap
	// --output-tree-parsimony=FILE, --output-tree-mutations=FILE, --output-tree-sites=FILE (with --output-tree): Fitch's parsimony of the SNP
	// sites on that tree, from v2m_tree_parsimony
	char const *output_tree_parsimony{}, *output_tree_mutations{}, *output_tree_sites{};
	std::uint64_t tree_seed_value{1};
	bool all_columns{};                   // --all-columns (with --output-column-counts): every column, not only the variable ones
	// --output-diversity=FILE, --diversity-sfs=FILE, --output-divergence=FILE: windowed diversity, the folded spectrum and the divergence
	// between groups, from v2m_window_diversity / v2m_diversity_of_counts; --diversity-window=BP, --diversity-step=BP, --diversity-groups=FILE
	char const *output_diversity{}, *diversity_sfs{}, *output_divergence{}, *diversity_window{}, *diversity_step{}, *diversity_groups{};
	std::uint64_t diversity_window_bp{10000}, diversity_step_bp{10000};
	std::vector<std::pair<std::string, std::string>> diversity_group_of;
	bool distinct{};                      // --distinct (with --regions-file): every distinct sequence of a region once, and <name>.classes.tsv
	std::vector<int> devices{0};
};

// Reads --diversity-groups: a TSV of sequence id and group name a line; empty lines and lines that begin with '#' are skipped.  Returns
// an error text, or the empty string.  More than 16 groups, a line without two fields and an id named twice are errors here; an id that
// names no output sequence is one once the sequences are known.
std::string read_groups_file(char const *path, std::vector<std::pair<std::string, std::string>> &group_of)
{
	std::ifstream in(path);
	if (!in) return std::string("unable to open ") + path;
	std::set<std::string> ids, groups;
	std::string line;
	std::size_t number(0);
	while (std::getline(in, line)) {
		++number;
		if (!line.empty() && '\r' == line.back()) line.pop_back();
		if (line.empty() || '#' == line[0]) continue;
		auto const tab(line.find('\t'));
		if (std::string::npos == tab || 0 == tab || tab + 1 == line.size() || std::string::npos != line.find('\t', tab + 1))
			return std::string(path) + ", line " + std::to_string(number) + ": a line holds a sequence id, a tab and a group name";
		std::string const id(line.substr(0, tab)), group(line.substr(tab + 1));
		if (!ids.insert(id).second) return std::string(path) + ", line " + std::to_string(number) + ": \"" + id + "\" is named twice";
		groups.insert(group);
		if (groups.size() > 16) return std::string(path) + ", line " + std::to_string(number) + ": more than 16 groups";
		group_of.emplace_back(id, group);
	}
	if (group_of.empty()) return std::string(path) + " names no sequence";
	return std::string();
}

// The first id of group_of that is neither [prefix.]REF nor [prefix.]<sample>.<number> for a sample of the #CHROM line of the plain-text
// VCF at `path`; the empty string when there is none, or when the file is compressed, cannot be read or has no such line.
std::string unknown_group_id(char const *path, char const *chromosome_prefix, std::vector<std::pair<std::string, std::string>> const &group_of)
{
	std::ifstream in(path, std::ios::binary);
	if (!in || 0x1f == in.peek()) return std::string();
	std::set<std::string> samples;
	std::string line;
	bool found(false);
	while (std::getline(in, line)) {
		if (line.empty() || '#' != line[0]) break;
		if (0 != line.compare(0, 6, "#CHROM")) continue;
		if ('\r' == line.back()) line.pop_back();
		std::istringstream fields(line);
		std::string field;
		for (int k(0); std::getline(fields, field, '\t'); ++k) if (k >= 9) samples.insert(field);
		found = true;
		break;
	}
	if (!found) return std::string();
	std::string const prefix(chromosome_prefix ? std::string(chromosome_prefix) + '.' : std::string());
	for (auto const &[id, group] : group_of) {
		if (0 != id.compare(0, prefix.size(), prefix)) return id;
		std::string const name(id.substr(prefix.size()));
		if ("REF" == name) continue;
		auto const dot(name.rfind('.'));
		if (std::string::npos == dot || dot + 1 == name.size() || std::string::npos != name.find_first_not_of("0123456789", dot + 1) || !samples.count(name.substr(0, dot))) return id;
	}
	return std::string();
}

void usage()
{
	std::cerr <<
		"Usage: vcf2multialign --haplotypes --input-reference=filename.fa --input-variants=filename.vcf --chromosome=id [<options>]\n"
		"  -H, --haplotypes                   Produce predicted haplotype sequences\n"
		"  -r, --input-reference=filename     Reference FASTA file path (plain or BGZF)\n"
		"  -e, --reference-sequence=id        Reference sequence identifier in the input FASTA\n"
		"  -a, --input-variants=filename      Variant call file path (plain or BGZF)\n"
		"  -c, --chromosome=id                Chromosome identifier\n"
		"  -s, --output-sequences-a2m=file    Output reference-guided multiple alignment as A2M\n"
		"      --output-sequences-separate    Output one sequence per file\n"
		"      --separate-output-format=fmt   A2M (default) or plain\n"
		"  -m, --dst-chromosome=id            Chromosome identifier in output\n"
		"      --omit-reference               Omit the reference sequence from the output\n"
		"      --unaligned                    Output unaligned sequences instead of an MSA\n"
		"      --output-overlaps=file         Output overlapping variants as TSV instead of stdout\n"
		"      --output-graph-statistics      Output graph statistics to stdout\n"
		"      --ref-mismatch-handling=how    warning (default) or error\n"
		"      --include-samples=file         TSV (chrom, sample, copy_idx) of the only copies to include\n"
		"  -x, --exclude-samples=file         TSV (chrom, sample, copy_idx) of copies to exclude\n"
		"      --device=n[,m...]              HIP device(s) to run on (default 0); with several, the rows of an aligned\n"
		"                                     A2M file are sharded over them (graph replicated, no collective)\n"
		"      --bgzf                         Write the A2M file (-s) as BGZF, compressed on the GPU (gzip -d or any BGZF\n"
		"                                     reader gives the plain A2M back; not with --pipe or --output-sequences-separate)\n"
		"      --region=START-END             Output only the alignment columns of reference positions START..END (1-based,\n"
		"                                     inclusive, as in samtools/bcftools), with the insertions anchored there\n"
		"      --regions-file=FILE.bed        Write one file per BED region (chrom, 0-based start, exclusive end, optional name;\n"
		"                                     tab-separated) into the working directory: <name>.a2m, or <name>.fa with --unaligned,\n"
		"                                     each holding every sequence cut to the region as -s with --region=<start+1>-<end>\n"
		"                                     would write it.  Lines of other chromosomes than --chromosome are skipped; a region\n"
		"                                     without a name is called <chrom>_<start>_<end>.  All regions are spliced together,\n"
		"                                     one launch per row batch.  Not with --region, -s, --output-sequences-separate,\n"
		"                                     --pipe, --bgzf or several --device entries\n"
		"      --distinct                     With --regions-file: write every distinct sequence of a region once -- the region's file\n"
		"                                     without the records whose sequence occurred earlier in it -- and <name>.classes.tsv with a\n"
		"                                     line per sequence: its identifier, the identifier of the first sequence equal to it, and\n"
		"                                     that one's index in the file.  The duplicates are found on the GPU and never leave it\n"
		"      --output-chain=FILE            Write one UCSC chain per output sequence (the reference as target, the sequence as\n"
		"                                     query; names as --output-sequences-separate forms them) that maps reference positions\n"
		"                                     to positions in the --unaligned sequence, e.g. for liftOver or CrossMap.  The REF row\n"
		"                                     has no chain.  Alone or beside -s / --output-sequences-separate; not with --region,\n"
		"                                     --regions-file or several --device entries\n"
		"      --output-paf=FILE              Write one PAF line per output sequence (the sequence as query, the reference as target;\n"
		"                                     names as for --output-chain) with the number of matching bytes, NM and the extended\n"
		"                                     CIGAR (cg:Z: in = X I D, as minimap2 --eqx -c writes it): where the sequence differs\n"
		"                                     from the reference.  Letters compare without case.  The REF row has no line.  Alone\n"
		"                                     or beside -s / --output-sequences-separate / --output-chain; not with --region,\n"
		"                                     --regions-file or several --device entries\n"
		"      --output-column-counts=FILE    Write a TSV with one line per variable alignment column: the 0-based column, the 1-based\n"
		"                                     reference position (`.` where the reference has padding) and how many of the output\n"
		"                                     sequences (REF first, unless --omit-reference) hold A, C, G, T, N (either case), a gap or\n"
		"                                     another byte there, counted on the GPU.  Always of the aligned form, whatever --unaligned\n"
		"                                     says; --region restricts the columns.  Alone or beside -s / --output-sequences-separate /\n"
		"                                     --output-chain / --output-paf; not with --regions-file or several --device entries\n"
		"      --all-columns                  With --output-column-counts: write every column, not only the variable ones\n"
		"      --output-distances=FILE        Write a TSV with the matrix of pairwise distances between the output sequences (REF first,\n"
		"                                     unless --omit-reference), as snp-dists writes it: a `#rows` line, a header line with the\n"
		"                                     sequence names (those of --output-paf), then one line per sequence.  A distance is the\n"
		"                                     number of alignment columns in which two sequences differ by class (A, C, G, T, N -- either\n"
		"                                     case --, gap, other), counted on the GPU.  Always of the aligned form, whatever --unaligned\n"
		"                                     says; --region restricts the columns.  Alone or beside the other outputs; not with\n"
		"                                     --regions-file or several --device entries\n"
		"      --acgt-only                    With --output-distances: count only the columns where both sequences hold A, C, G or T\n"
		"      --output-variable-sites=FILE   Write a FASTA file with the output sequences (REF first, unless --omit-reference) cut down\n"
		"                                     to the variable alignment columns, gathered on the GPU: the -s file with every sequence\n"
		"                                     line reduced to the columns in which the sequences differ by class (A, C, G, T, N --\n"
		"                                     either case --, gap, other), as snp-sites makes it from a multi-FASTA.  Always of the\n"
		"                                     aligned form, whatever --unaligned says; --region restricts the columns.  Alone or beside\n"
		"                                     the other outputs; not with --regions-file or several --device entries\n"
		"      --snp-sites                    With --output-variable-sites: keep only the columns where at least two of A, C, G, T\n"
		"                                     occur (snp-sites' rule); columns that vary only by gap, N or other bytes are left out\n"
		"      --output-site-positions=FILE   With --output-variable-sites: write one line per kept column, `column<TAB>reference\n"
		"                                     position` (the first two fields of its --output-column-counts line)\n"
		"      --output-ld=FILE               Write a TSV with the linkage disequilibrium between nearby biallelic sites of the output\n"
		"                                     sequences (REF first, unless --omit-reference), as plink --r2 reports it for phased\n"
		"                                     haplotypes: a `#rows` line, a header line, then per reported pair of sites the column and\n"
		"                                     reference position of both, the sequences called at both (n), those that carry the\n"
		"                                     second allele at the first site, at the second, and at both, and r2.  A site is a\n"
		"                                     column where exactly two of A, C, G, T occur; sequences that hold anything else there are\n"
		"                                     missing.  Counted on the GPU.  Always of the aligned form, whatever --unaligned says;\n"
		"                                     --region restricts the columns.  Alone or beside the other outputs; not with\n"
		"                                     --regions-file or several --device entries\n"
		"      --ld-window=SITES              With --output-ld: pairs at most SITES sites apart (1 to 4096; default 1000)\n"
		"      --ld-window-columns=N          With --output-ld: pairs at most N alignment columns apart (default 0: no limit)\n"
		"      --ld-min-r2=DECIMAL            With --output-ld: report the pairs with r2 >= DECIMAL (0 to 1, at most 6 decimals;\n"
		"                                     default 0.2), compared exactly\n"
		"      --ld-min-count=N               With --output-ld: a site's two alleles each occur at least N times (default 1)\n"
		"      --output-tree=FILE             Write the neighbour-joining tree of the output sequences (REF first, unless\n"
		"                                     --omit-reference; at least three) in Newick form: canonical NJ on the matrix of\n"
		"                                     --output-distances, unrooted (the last three nodes meet in a trifurcation), leaves named as\n"
		"                                     --output-distances names them, branch lengths in columns, negative ones kept.  Distances and\n"
		"                                     tree are computed on the GPU, in IEEE double precision without fused multiply-adds, ties\n"
		"                                     broken by node number.  Always of the aligned form, whatever --unaligned says; --region\n"
		"                                     restricts the columns.  Alone or beside the other outputs; not with --regions-file or\n"
		"                                     several --device entries\n"
		"      --tree-acgt-only               With --output-tree: the distances count only the columns where both sequences hold A, C, G\n"
		"                                     or T (as --acgt-only does for --output-distances)\n"
		"      --tree-bootstrap=B             With --output-tree: Felsenstein's bootstrap.  The columns are resampled with replacement B\n"
		"                                     times (1 to 100000) on the GPU, the tree is built again from every replicate, and each\n"
		"                                     join of the tree is labelled with the number of replicates that hold its split\n"
		"      --tree-seed=S                  With --tree-bootstrap: the seed of the draws (0 to 2^64 - 1; default 1)\n"
		"      --output-tree-replicates=FILE  With --tree-bootstrap: write the replicate trees, one Newick line each (the input of\n"
		"                                     consense)\n"
		"      --output-tree-parsimony=FILE   With --output-tree: write the same tree in Newick form with every branch length the number\n"
		"                                     of changes Fitch's parsimony puts on the branch, over the SNP columns of the alignment\n"
		"                                     (A, C, G, T; anything else counts as missing), rooted at the trifurcation, and every\n"
		"                                     internal node labelled node<t> by its join.  Computed on the GPU, in integers\n"
		"      --output-tree-mutations=FILE   With --output-tree: write those changes, one line each: node (the sequence, or node<t>),\n"
		"                                     column, reference position (as --output-site-positions writes them), from, to\n"
		"      --output-tree-sites=FILE       With --output-tree: write one line per SNP column: column, reference position, the letters\n"
		"                                     present, the steps on the tree, and the homoplasy steps - (letters - 1)\n"
		"      --output-diversity=FILE        Write a TSV with one line per window of the reference and group of output sequences: group,\n"
		"                                     start, end (reference positions, 1-based inclusive), columns, called, diffs, pairs, pi,\n"
		"                                     segregating, complete, theta_w, tajima_d (nucleotide diversity, Watterson's theta and\n"
		"                                     Tajima's D; NA where a value does not exist).  Computed on the GPU from the column counts,\n"
		"                                     in integers; always of the aligned form; --region restricts the columns.  The columns of\n"
		"                                     an insertion fall to the window of the reference position before them.  Not with\n"
		"                                     --regions-file or several --device entries\n"
		"      --diversity-window=BP          The window, in reference positions (default 10000)\n"
		"      --diversity-step=BP            The step between window starts (default: the window); it must divide the window\n"
		"      --diversity-sfs=FILE           Write the folded site frequency spectrum of every group: group, n, minor count, columns\n"
		"      --diversity-groups=FILE        A TSV of sequence id (as --output-distances names them) and group name; a sequence it does\n"
		"                                     not name belongs to no group; at most 16 groups.  Without it there is one group, all\n"
		"      --output-divergence=FILE       With --diversity-groups: write per pair of groups and window group_a, group_b, start, end,\n"
		"                                     columns, called, diffs, pairs, dxy, fst (Hudson's)\n"
		"      --gpu-parse                    Parse the genotype columns of --input-variants on the first GPU, under the BGZF\n"
		"                                     inflate for compressed input: the VCF text never reaches the host (not with -g).\n"
		"                                     Input the scan does not support (more than 32 768 chromosome copies, a line longer\n"
		"                                     than a 64-MiB slice) is parsed on the host instead when that shows before the first\n"
		"                                     record is merged; a too-long line after that is an error\n"
		"      --verbose\n"
		"  BGZF input (bgzip, bcftools -Oz, a .fa.gz for samtools faidx) is recognised by its first bytes and inflated on the first\n"
		"  GPU; the decompressed text is held in host memory (as large as the text).  Plain gzip has to be recompressed with bgzip.\n"
		"  -F, --founder-sequences=count      Produce founder sequences instead of haplotypes\n"
		"  -d, --minimum-distance=distance    Minimum node distance (MSA co-ordinates) between cut positions\n"
		"      --keep-ref-edges               Take the reference edges into account when matching\n"
		"  -g, --input-graph=filename         Variant graph input (this build's flat V2MGRAF1 format)\n"
		"  -f, --output-graph=filename        Output the variant graph\n"
		"  -p, --input-cut-positions=file     Cut position input\n"
		"  -t, --output-cut-positions=file    Output the cut positions\n"
		"      --pipe=command                 Instead of writing sequences to files, pipe them to `command <name>`\n"
		"  (--output-graphviz and --output-memory-breakdown are outside this build's scope: SURVEY.md section 2)\n";
}

typedef std::set<std::tuple<std::string, std::string, unsigned>> sample_set;


// main.cc:42-120 (sample filter lists): TSV rows (chrom, sample, copy_idx)
sample_set read_sample_list(char const *path, char const *chromosome)
{
	sample_set out;
	std::ifstream is(path);
	if (!is) { std::cerr << "ERROR: Unable to open " << path << '\n'; std::exit(EXIT_FAILURE); }
	std::string line;
	while (std::getline(is, line)) {
		if (line.empty()) continue;
		std::istringstream ls(line);
		std::string chrom, sample; unsigned copy{};
		if (!(std::getline(ls, chrom, '\t') && std::getline(ls, sample, '\t') && (ls >> copy))) continue;
		if (chromosome && chrom != chromosome) continue;
		out.emplace(chrom, sample, copy);
	}
	return out;
}

struct build_delegate final : vh::build_graph_delegate {
	sample_set const *included{}, *excluded{};
	std::string chromosome;
	std::ostream *overlaps{&std::cout};
	bool mismatch_is_error{};
	bool is_tsv{};

	bool should_include(std::string_view sample_name, vh::u32 chrom_copy_idx) const override
	{
		auto const key(std::make_tuple(chromosome, std::string(sample_name), unsigned(chrom_copy_idx)));
		if (included) return included->count(key) > 0;
		if (excluded) return excluded->count(key) == 0;
		return true;
	}

	static std::string joined_ids(std::string_view var_id, char const *sep)
	{
		std::string out;   // the VCF ID column holds ';'-separated identifiers
		for (char const c : var_id) { if (';' == c) out += sep; else out.push_back(c); }
		return out;
	}

	void report_overlapping_alternative(vh::u64 lineno, vh::u64 ref_pos, std::string_view var_id, std::string_view sample_name, vh::u32 chrom_copy_idx, vh::u32 gt) override
	{
		if (is_tsv)   // main.cc:159-165
			*overlaps << lineno << '\t' << ref_pos << '\t' << joined_ids(var_id, ",") << '\t' << sample_name << '\t' << chrom_copy_idx << '\t' << gt << '\n';
		else          // main.cc:168-170
			*overlaps << "Overlapping alternative alleles. Line number: " << lineno << " current variant position: " << ref_pos
				<< " variant identifiers: " << joined_ids(var_id, ", ") << " sample: " << sample_name << " chromosome copy: " << chrom_copy_idx << " genotype: " << gt << '\n';
	}

	bool ref_column_mismatch(vh::u64 var_idx, vh::u64 ref_pos, std::string_view ref_in_vcf, std::string_view expected) override
	{
		std::cerr << (mismatch_is_error ? "ERROR: " : "WARNING: ") << "REF column contents do not match the reference sequence in variant " << var_idx
			<< ", position " << (1 + ref_pos) << ". Expected: \"" << expected << "\" Actual: \"" << ref_in_vcf << "\"\n";   // main.cc:179-189
		if (mismatch_is_error) std::exit(EXIT_FAILURE);
		return true;
	}
};

struct progress_delegate final : vh::output_delegate {
	bool verbose{};
	void will_handle_sample(std::string const &, vh::u32, vh::u32) override {}
	void will_handle_founder_sequence(vh::u32) override {}
	void handled_sequences(vh::u32 count) override
	{
		if (verbose && 0 == count % 10) std::cerr << "Handled " << count << " sequences...\n";   // main.cc:313-330
	}
};

// A decimal count: digits only, at most 18 of them.
bool parse_count(char const *text, std::uint64_t &out)
{
	std::string const t(text);
	if (t.empty() || t.size() > 18 || std::string::npos != t.find_first_not_of("0123456789")) return false;
	out = std::stoull(t);
	return true;
}

// A seed: decimal, 0 to 2^64 - 1.
bool parse_seed(char const *text, std::uint64_t &out)
{
	std::string const t(text);
	if (t.empty() || t.size() > 20 || std::string::npos != t.find_first_not_of("0123456789")) return false;
	errno = 0;
	out = std::strtoull(t.c_str(), nullptr, 10);
	return 0 == errno;
}

// --region's value: START-END, decimal, 1 <= START <= END (the reference length is checked once the reference is read).
bool parse_region(char const *text, std::uint64_t &start, std::uint64_t &end)
{
	std::string const s(text);
	auto const dash(s.find('-'));
	if (std::string::npos == dash) return false;
	auto const number([](std::string const &t, std::uint64_t &out) {
		if (t.empty() || t.size() > 18 || std::string::npos != t.find_first_not_of("0123456789")) return false;
		out = std::stoull(t);
		return true;
	});
	return number(s.substr(0, dash), start) && number(s.substr(dash + 1), end) && 1 <= start && start <= end;
}

// One region of --regions-file: reference range [start, end) (0-based, half-open) and the name of its output file.
struct bed_region {
	std::string name;
	std::uint64_t start{}, end{}, line{};
};

// Reads --regions-file.  Lines that are empty or start with '#', "track" or "browser" are skipped, and so are the lines of other
// chromosomes than `chromosome` (counted in skipped; without a chromosome every line is taken).  Returns an empty string, or what is
// wrong with the file -- with the line number where a line is at fault.
std::string read_regions_file(char const *path, char const *chromosome, std::uint64_t ref_len, std::vector<bed_region> &regions, std::uint64_t &skipped)
{
	std::ifstream is(path);
	if (!is) return std::string("unable to open ") + path;
	auto const at([&](std::uint64_t line, std::string const &what) { return std::string(path) + " line " + std::to_string(line) + ": " + what; });
	auto const number([](std::string const &t, std::uint64_t &out) {
		if (t.empty() || t.size() > 18 || std::string::npos != t.find_first_not_of("0123456789")) return false;
		out = std::stoull(t);
		return true;
	});
	std::map<std::string, std::uint64_t> seen;
	std::string text;
	skipped = 0;
	for (std::uint64_t line(1); std::getline(is, text); ++line) {
		if (!text.empty() && '\r' == text.back()) text.pop_back();
		if (text.empty() || '#' == text[0] || 0 == text.compare(0, 5, "track") || 0 == text.compare(0, 7, "browser")) continue;
		std::vector<std::string> fields;
		for (std::size_t pos(0);;) {
			auto const tab(text.find('\t', pos));
			fields.push_back(text.substr(pos, std::string::npos == tab ? tab : tab - pos));
			if (std::string::npos == tab) break;
			pos = tab + 1;
		}
		if (fields.size() < 3) return at(line, "a region needs at least three tab-separated fields (chrom, start, end)");
		if (chromosome && fields[0] != chromosome) { ++skipped; continue; }
		bed_region r;
		r.line = line;
		if (!number(fields[1], r.start) || !number(fields[2], r.end)) return at(line, "start and end must be non-negative decimal integers, got \"" + fields[1] + "\" and \"" + fields[2] + "\"");
		if (r.start >= r.end) return at(line, "start " + fields[1] + " is not less than end " + fields[2] + " (0-based start, exclusive end)");
		if (r.end > ref_len) return at(line, "end " + fields[2] + " is past the end of the reference sequence (" + std::to_string(ref_len) + ")");
		r.name = fields.size() >= 4 ? fields[3] : fields[0] + "_" + fields[1] + "_" + fields[2];
		if (r.name.empty() || "." == r.name || ".." == r.name || std::string::npos != r.name.find('/') || std::string::npos != r.name.find('\0'))
			return at(line, "region name \"" + r.name + "\" cannot name a file (empty, \".\", \"..\", or holding '/' or NUL)");
		auto const ins(seen.emplace(r.name, line));
		if (!ins.second) return at(line, "duplicate region name \"" + r.name + "\" (first on line " + std::to_string(ins.first->second) + ")");
		regions.push_back(std::move(r));
	}
	if (regions.empty())
		return std::string(path) + (chromosome && skipped ? std::string(" holds no region on chromosome \"") + chromosome + "\"" : std::string(" holds no region"));
	return {};
}

// Regions per pass of --regions-file: one file is open per region, so as many as the process may have open -- the soft limit is raised
// to the hard one -- less a margin for everything else it holds --, divided by the files a region takes (two with --distinct).
// V2M_REGIONS_PER_PASS overrides (tests).
std::size_t regions_per_pass(std::size_t files_per_region)
{
	char const *const e(std::getenv("V2M_REGIONS_PER_PASS"));
	if (e && *e && std::atol(e) > 0) return std::size_t(std::atol(e));
	struct rlimit lim{};
	if (0 != ::getrlimit(RLIMIT_NOFILE, &lim)) return 192;
	if (lim.rlim_cur != lim.rlim_max) {
		struct rlimit raised(lim);
		raised.rlim_cur = RLIM_INFINITY == lim.rlim_max ? rlim_t(1) << 20 : lim.rlim_max;
		if (0 == ::setrlimit(RLIMIT_NOFILE, &raised)) lim = raised;
	}
	rlim_t const margin(64);
	return (RLIM_INFINITY == lim.rlim_cur ? (std::size_t(1) << 20) : lim.rlim_cur > 2 * margin ? std::size_t(lim.rlim_cur - margin) : std::size_t(margin)) / files_per_region;
}

} // namespace


int main(int argc, char **argv)
{
	::signal(SIGPIPE, SIG_IGN);   // main.cc:372: a --pipe child that goes away shows up as a write error
	// A command-line run is one shot: the library's per-context calibrations (which transpose kernel for a matrix shape, plain
	// or nontemporal row stores: a handful of extra launches each) have nothing to amortise over, so the driver presets what
	// they choose on nearly every box.  A value already in the environment wins.
	::setenv("V2M_TRANSPOSE_PANEL", "stream16", 0);
	::setenv("V2M_NT_STORES", "1", 0);
	::setenv("V2M_UNALIGNED_STORE", "plain", 0);
	options opt;
	enum { o_keep_ref = 900, o_separate = 1000, o_sep_format, o_omit_ref, o_unaligned, o_overlaps, o_stats, o_mismatch, o_include, o_device, o_verbose, o_pipe, o_bgzf, o_region, o_gpu_parse, o_regions_file, o_output_chain, o_distinct, o_output_paf, o_output_column_counts, o_all_columns, o_output_distances, o_acgt_only, o_output_variable_sites, o_snp_sites, o_output_site_positions, o_output_ld, o_ld_window, o_ld_window_columns, o_ld_min_r2, o_ld_min_count, o_output_tree, o_tree_acgt_only, o_tree_bootstrap, o_tree_seed, o_output_tree_replicates, o_output_tree_parsimony, o_output_tree_mutations, o_output_tree_sites, o_output_diversity, o_diversity_window, o_diversity_step, o_diversity_sfs, o_diversity_groups, o_output_divergence, o_unsupported };
	static option const longopts[] = {
		{"haplotypes", no_argument, nullptr, 'H'}, {"founder-sequences", required_argument, nullptr, 'F'},
		{"input-reference", required_argument, nullptr, 'r'}, {"reference-sequence", required_argument, nullptr, 'e'},
		{"input-variants", required_argument, nullptr, 'a'}, {"chromosome", required_argument, nullptr, 'c'},
		{"output-sequences-a2m", required_argument, nullptr, 's'}, {"output-sequences-separate", no_argument, nullptr, o_separate},
		{"separate-output-format", required_argument, nullptr, o_sep_format}, {"dst-chromosome", required_argument, nullptr, 'm'},
		{"omit-reference", no_argument, nullptr, o_omit_ref}, {"unaligned", no_argument, nullptr, o_unaligned},
		{"output-overlaps", required_argument, nullptr, o_overlaps}, {"output-graph-statistics", no_argument, nullptr, o_stats},
		{"ref-mismatch-handling", required_argument, nullptr, o_mismatch}, {"include-samples", required_argument, nullptr, o_include},
		{"exclude-samples", required_argument, nullptr, 'x'}, {"device", required_argument, nullptr, o_device}, {"verbose", no_argument, nullptr, o_verbose},
		{"input-graph", required_argument, nullptr, 'g'}, {"output-graph", required_argument, nullptr, 'f'},
		{"output-graphviz", required_argument, nullptr, o_unsupported}, {"output-memory-breakdown", required_argument, nullptr, o_unsupported}, {"pipe", required_argument, nullptr, o_pipe}, {"bgzf", no_argument, nullptr, o_bgzf}, {"region", required_argument, nullptr, o_region}, {"gpu-parse", no_argument, nullptr, o_gpu_parse}, {"regions-file", required_argument, nullptr, o_regions_file}, {"output-chain", required_argument, nullptr, o_output_chain}, {"distinct", no_argument, nullptr, o_distinct}, {"output-paf", required_argument, nullptr, o_output_paf}, {"output-column-counts", required_argument, nullptr, o_output_column_counts}, {"all-columns", no_argument, nullptr, o_all_columns}, {"output-distances", required_argument, nullptr, o_output_distances}, {"acgt-only", no_argument, nullptr, o_acgt_only}, {"output-variable-sites", required_argument, nullptr, o_output_variable_sites}, {"snp-sites", no_argument, nullptr, o_snp_sites}, {"output-site-positions", required_argument, nullptr, o_output_site_positions},
		{"output-ld", required_argument, nullptr, o_output_ld}, {"ld-window", required_argument, nullptr, o_ld_window}, {"ld-window-columns", required_argument, nullptr, o_ld_window_columns},
		{"ld-min-r2", required_argument, nullptr, o_ld_min_r2}, {"ld-min-count", required_argument, nullptr, o_ld_min_count},
		{"output-tree", required_argument, nullptr, o_output_tree}, {"tree-acgt-only", no_argument, nullptr, o_tree_acgt_only},
		{"tree-bootstrap", required_argument, nullptr, o_tree_bootstrap}, {"tree-seed", required_argument, nullptr, o_tree_seed}, {"output-tree-replicates", required_argument, nullptr, o_output_tree_replicates},
		{"output-tree-parsimony", required_argument, nullptr, o_output_tree_parsimony}, {"output-tree-mutations", required_argument, nullptr, o_output_tree_mutations},
		{"output-tree-sites", required_argument, nullptr, o_output_tree_sites},
		{"output-diversity", required_argument, nullptr, o_output_diversity}, {"diversity-window", required_argument, nullptr, o_diversity_window},
		{"diversity-step", required_argument, nullptr, o_diversity_step}, {"diversity-sfs", required_argument, nullptr, o_diversity_sfs},
		{"diversity-groups", required_argument, nullptr, o_diversity_groups}, {"output-divergence", required_argument, nullptr, o_output_divergence},
		{"minimum-distance", required_argument, nullptr, 'd'}, {"input-cut-positions", required_argument, nullptr, 'p'},
		{"output-cut-positions", required_argument, nullptr, 't'}, {"keep-ref-edges", no_argument, nullptr, o_keep_ref},
		{"help", no_argument, nullptr, 'h'}, {nullptr, 0, nullptr, 0}};
	int c;
	while (-1 != (c = getopt_long(argc, argv, "HF:d:p:t:r:e:a:c:s:m:x:g:f:v:h", longopts, nullptr))) {
		switch (c) {
			case 'H': opt.haplotypes = true; break;
			case 'F': opt.founder_mode = true; opt.founder_sequences = std::atol(optarg); break;
			case 'd': opt.minimum_distance = std::atol(optarg); break;
			case o_keep_ref: opt.keep_ref_edges = true; break;
			case 'r': opt.input_reference = optarg; break;
			case 'e': opt.reference_sequence = optarg; break;
			case 'a': opt.input_variants = optarg; break;
			case 'c': opt.chromosome = optarg; break;
			case 's': opt.output_sequences_a2m = optarg; break;
			case 'm': opt.dst_chromosome = optarg; break;
			case 'x': opt.exclude_samples = optarg; break;
			case 'g': opt.input_graph = optarg; break;
			case 'f': opt.output_graph = optarg; break;
			case o_separate: opt.output_sequences_separate = true; break;
			case o_sep_format:
				if (0 == std::strcmp(optarg, "plain")) opt.separate_plain = true;
				else if (0 != std::strcmp(optarg, "A2M")) { std::cerr << "ERROR: --separate-output-format must be A2M or plain.\n"; return EXIT_FAILURE; }
				break;
			case o_omit_ref: opt.omit_reference = true; break;
			case o_unaligned: opt.unaligned = true; break;
			case o_overlaps: opt.output_overlaps = optarg; break;
			case o_stats: opt.graph_statistics = true; break;
			case o_mismatch:
				if (0 == std::strcmp(optarg, "error")) opt.ref_mismatch_error = true;
				else if (0 != std::strcmp(optarg, "warning")) { std::cerr << "ERROR: --ref-mismatch-handling must be warning or error.\n"; return EXIT_FAILURE; }
				break;
			case o_include: opt.include_samples = optarg; break;
			case o_device: {
				opt.devices.clear();
				std::istringstream ds(optarg);
				for (std::string tok; std::getline(ds, tok, ',');) if (!tok.empty()) opt.devices.push_back(std::atoi(tok.c_str()));
				if (opt.devices.empty()) { std::cerr << "ERROR: --device needs at least one device.\n"; return EXIT_FAILURE; }
				break;
			}
			case o_verbose: opt.verbose = true; break;
			case o_pipe: opt.pipe = optarg; break;
			case o_bgzf: opt.bgzf = true; break;
			case o_gpu_parse: opt.gpu_parse = true; break;
			case o_region: opt.region = optarg; break;
			case o_regions_file: opt.regions_file = optarg; break;
			case o_output_chain: opt.output_chain = optarg; break;
			case o_distinct: opt.distinct = true; break;
			case o_output_paf: opt.output_paf = optarg; break;
			case o_output_column_counts: opt.output_column_counts = optarg; break;
			case o_all_columns: opt.all_columns = true; break;
			case o_output_distances: opt.output_distances = optarg; break;
			case o_acgt_only: opt.acgt_only = true; break;
			case o_output_variable_sites: opt.output_variable_sites = optarg; break;
			case o_snp_sites: opt.snp_sites = true; break;
			case o_output_site_positions: opt.output_site_positions = optarg; break;
			case o_output_ld: opt.output_ld = optarg; break;
			case o_ld_window: opt.ld_window = optarg; break;
			case o_ld_window_columns: opt.ld_window_columns = optarg; break;
			case o_ld_min_r2: opt.ld_min_r2 = optarg; break;
			case o_ld_min_count: opt.ld_min_count = optarg; break;
			case o_output_tree: opt.output_tree = optarg; break;
			case o_tree_acgt_only: opt.tree_acgt_only = true; break;
			case o_tree_bootstrap: opt.tree_bootstrap = optarg; break;
			case o_tree_seed: opt.tree_seed = optarg; break;
			case o_output_tree_replicates: opt.output_tree_replicates = optarg; break;
			case o_output_tree_parsimony: opt.output_tree_parsimony = optarg; break;
			case o_output_tree_mutations: opt.output_tree_mutations = optarg; break;
			case o_output_tree_sites: opt.output_tree_sites = optarg; break;
			case o_output_diversity: opt.output_diversity = optarg; break;
			case o_diversity_window: opt.diversity_window = optarg; break;
			case o_diversity_step: opt.diversity_step = optarg; break;
			case o_diversity_sfs: opt.diversity_sfs = optarg; break;
			case o_diversity_groups: opt.diversity_groups = optarg; break;
			case o_output_divergence: opt.output_divergence = optarg; break;
			case 'p': opt.input_cut_positions = optarg; break;
			case 't': opt.output_cut_positions = optarg; break;
			case 'h': usage(); return EXIT_SUCCESS;
			case 'v':   // --output-graphviz's short form (cmdline.ggo:38): the same answer
			case o_unsupported: std::cerr << "ERROR: option " << ('v' == c ? "-v / --output-graphviz" : argv[optind - 1]) << " is not supported by this build.\n"; return EXIT_FAILURE;
			default: usage(); return EXIT_FAILURE;
		}
	}

	// main.cc:577-611
	if (opt.haplotypes == opt.founder_mode) { std::cerr << "ERROR: exactly one of --haplotypes and --founder-sequences is required.\n"; return EXIT_FAILURE; }
	if (opt.founder_mode && opt.founder_sequences <= 0) { std::cerr << "ERROR: --founder-sequences must be positive.\n"; return EXIT_FAILURE; }   // main.cc:595-599
	if (opt.minimum_distance < 0) { std::cerr << "ERROR: --minimum-distance must be non-negative.\n"; return EXIT_FAILURE; }                    // main.cc:607-611
	if (!opt.input_reference) { std::cerr << "ERROR: --input-reference is required.\n"; return EXIT_FAILURE; }
	if (opt.input_variants && opt.input_graph) { std::cerr << "ERROR: Only one of --input-variants and --input-graph can be specified.\n"; return EXIT_FAILURE; }   // main.cc:577-581
	if (!opt.input_variants && !opt.input_graph) { std::cerr << "ERROR: One of --input-variants and --input-graph must be specified.\n"; return EXIT_FAILURE; }  // main.cc:583-587
	if (opt.input_variants && !opt.chromosome) { std::cerr << "ERROR: --chromosome must be specified with --input-variants.\n"; return EXIT_FAILURE; }          // main.cc:589-593
	if (opt.output_graph && !opt.input_variants) { std::cerr << "ERROR: --output-graph requires --input-variants.\n"; return EXIT_FAILURE; }                     // cmdline.ggo:40 (dependon)
	if (opt.include_samples && opt.exclude_samples) { std::cerr << "ERROR: --include-samples and --exclude-samples are mutually exclusive.\n"; return EXIT_FAILURE; }
	// --bgzf compresses the one A2M file; a pipe's command already is the user's compressor, one file per sequence is out of its scope
	if (opt.bgzf && !opt.output_sequences_a2m) { std::cerr << "ERROR: --bgzf requires -s / --output-sequences-a2m.\n"; return EXIT_FAILURE; }
	if (opt.bgzf && opt.pipe) { std::cerr << "ERROR: --bgzf cannot be combined with --pipe (the piped command compresses).\n"; return EXIT_FAILURE; }
	if (opt.bgzf && opt.output_sequences_separate) { std::cerr << "ERROR: --bgzf cannot be combined with --output-sequences-separate.\n"; return EXIT_FAILURE; }
	if (opt.gpu_parse && !opt.input_variants) { std::cerr << "ERROR: --gpu-parse parses --input-variants; it cannot be combined with --input-graph.\n"; return EXIT_FAILURE; }
	if (opt.distinct && !opt.regions_file) { std::cerr << "ERROR: --distinct requires --regions-file.\n"; return EXIT_FAILURE; }
	if (opt.regions_file) {
		// one file per region, written by one context from one window set per pass: the other ways out do not apply
		char const *const other(opt.region ? "--region" : opt.output_sequences_a2m ? "-s / --output-sequences-a2m" : opt.output_sequences_separate ? "--output-sequences-separate"
			: opt.pipe ? "--pipe" : opt.bgzf ? "--bgzf" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --regions-file cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
	}
	if (opt.output_chain) {
		// a chain describes whole rows, from one context that holds every chromosome copy
		char const *const other(opt.region ? "--region" : opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-chain cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
	}
	if (opt.output_paf) {
		// as for a chain: whole rows, one context
		char const *const other(opt.region ? "--region" : opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-paf cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
	}
	if (opt.all_columns && !opt.output_column_counts) { std::cerr << "ERROR: --all-columns requires --output-column-counts.\n"; return EXIT_FAILURE; }
	if (opt.output_column_counts) {
		// one table from one context that holds every chromosome copy; a column window is fine, a window set is not a view of its own
		char const *const other(opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-column-counts cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
	}
	if (opt.acgt_only && !opt.output_distances) { std::cerr << "ERROR: --acgt-only requires --output-distances.\n"; return EXIT_FAILURE; }
	if (opt.output_distances) {
		// one matrix from one context that holds every chromosome copy; a column window is fine, a window set is not a view of its own
		char const *const other(opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-distances cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
	}
	{
		bool const any(opt.output_diversity || opt.diversity_sfs || opt.output_divergence);
		for (auto const &[value, name] : {std::pair<char const *, char const *>{opt.diversity_window, "--diversity-window"}, {opt.diversity_step, "--diversity-step"},
			{opt.diversity_groups, "--diversity-groups"}})
			if (value && !any) { std::cerr << "ERROR: " << name << " requires --output-diversity, --diversity-sfs or --output-divergence.\n"; return EXIT_FAILURE; }
		if (opt.output_divergence && !opt.diversity_groups) { std::cerr << "ERROR: --output-divergence requires --diversity-groups.\n"; return EXIT_FAILURE; }
		if (any) {
			char const *const other(opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
			if (other) { std::cerr << "ERROR: the diversity outputs cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
			if (opt.diversity_window && (!parse_count(opt.diversity_window, opt.diversity_window_bp) || 0 == opt.diversity_window_bp)) {
				std::cerr << "ERROR: --diversity-window must be a positive number of reference positions, got \"" << opt.diversity_window << "\".\n";
				return EXIT_FAILURE;
			}
			opt.diversity_step_bp = opt.diversity_window_bp;
			if (opt.diversity_step && (!parse_count(opt.diversity_step, opt.diversity_step_bp) || 0 == opt.diversity_step_bp)) {
				std::cerr << "ERROR: --diversity-step must be a positive number of reference positions, got \"" << opt.diversity_step << "\".\n";
				return EXIT_FAILURE;
			}
			if (opt.diversity_window_bp % opt.diversity_step_bp) {
				std::cerr << "ERROR: --diversity-step must divide --diversity-window (" << opt.diversity_window_bp << " is no multiple of " << opt.diversity_step_bp << ").\n";
				return EXIT_FAILURE;
			}
			if (opt.diversity_groups) {
				std::string const err(read_groups_file(opt.diversity_groups, opt.diversity_group_of));
				if (!err.empty()) { std::cerr << "ERROR: " << err << ".\n"; return EXIT_FAILURE; }
				// An id that can name no output sequence is refused before a device is opened, where the sample names can be read without one:
				// from the #CHROM line of a plain-text VCF.  The copy numbers, and compressed or graph input, are checked once the graph is built.
				if (opt.haplotypes && opt.input_variants) {
					std::string const bad(unknown_group_id(opt.input_variants, opt.dst_chromosome, opt.diversity_group_of));
					if (!bad.empty()) { std::cerr << "ERROR: " << opt.diversity_groups << ": \"" << bad << "\" names no output sequence.\n"; return EXIT_FAILURE; }
				}
			}
		}
	}
	if (opt.tree_acgt_only && !opt.output_tree) { std::cerr << "ERROR: --tree-acgt-only requires --output-tree.\n"; return EXIT_FAILURE; }
	if (opt.tree_bootstrap && !opt.output_tree) { std::cerr << "ERROR: --tree-bootstrap requires --output-tree.\n"; return EXIT_FAILURE; }
	if (opt.tree_seed && !opt.tree_bootstrap) { std::cerr << "ERROR: --tree-seed requires --tree-bootstrap.\n"; return EXIT_FAILURE; }
	if (opt.output_tree_replicates && !opt.tree_bootstrap) { std::cerr << "ERROR: --output-tree-replicates requires --tree-bootstrap.\n"; return EXIT_FAILURE; }
	for (auto const &[name, value] : {std::pair<char const *, char const *>{"--output-tree-parsimony", opt.output_tree_parsimony}, {"--output-tree-mutations", opt.output_tree_mutations},
		{"--output-tree-sites", opt.output_tree_sites}}) {
		if (value && !opt.output_tree) { std::cerr << "ERROR: " << name << " requires --output-tree.\n"; return EXIT_FAILURE; }
	}
	if (opt.tree_bootstrap) {
		std::uint64_t value(0);
		if (!parse_count(opt.tree_bootstrap, value) || value < 1 || value > V2M_NJ_BOOTSTRAP_MAX_REPLICATES) {
			std::cerr << "ERROR: --tree-bootstrap must be a number of replicates from 1 to " << V2M_NJ_BOOTSTRAP_MAX_REPLICATES << ", got \"" << opt.tree_bootstrap << "\".\n";
			return EXIT_FAILURE;
		}
		opt.tree_replicates = std::uint32_t(value);
		if (opt.tree_seed && !parse_seed(opt.tree_seed, opt.tree_seed_value)) {
			std::cerr << "ERROR: --tree-seed must be a number from 0 to 18446744073709551615, got \"" << opt.tree_seed << "\".\n";
			return EXIT_FAILURE;
		}
	}
	if (opt.output_tree) {
		// one matrix and one tree from one context that holds every chromosome copy; a column window is fine, a window set is not a view of its own
		char const *const other(opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-tree cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
		// the founder rows are counted here; the haplotype rows once the graph is there
		if (opt.founder_mode && opt.founder_sequences + (opt.omit_reference ? 0 : 1) < 3) {
			std::cerr << "ERROR: --output-tree needs at least three sequences (got " << opt.founder_sequences + (opt.omit_reference ? 0 : 1) << ").\n";
			return EXIT_FAILURE;
		}
	}
	if (opt.snp_sites && !opt.output_variable_sites) { std::cerr << "ERROR: --snp-sites requires --output-variable-sites.\n"; return EXIT_FAILURE; }
	if (opt.output_site_positions && !opt.output_variable_sites) { std::cerr << "ERROR: --output-site-positions requires --output-variable-sites.\n"; return EXIT_FAILURE; }
	if (opt.output_variable_sites) {
		// one set of sites from one context that holds every chromosome copy; a column window is fine, a window set is not a view of its own
		char const *const other(opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-variable-sites cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
	}
	for (auto const &[value, name] : {std::pair<char const *, char const *>{opt.ld_window, "--ld-window"}, {opt.ld_window_columns, "--ld-window-columns"}, {opt.ld_min_r2, "--ld-min-r2"}, {opt.ld_min_count, "--ld-min-count"}})
		if (value && !opt.output_ld) { std::cerr << "ERROR: " << name << " requires --output-ld.\n"; return EXIT_FAILURE; }
	if (opt.output_ld) {
		// one set of sites from one context that holds every chromosome copy; a column window is fine, a window set is not a view of its own
		char const *const other(opt.regions_file ? "--regions-file" : opt.devices.size() > 1 ? "more than one --device entry" : nullptr);
		if (other) { std::cerr << "ERROR: --output-ld cannot be combined with " << other << ".\n"; return EXIT_FAILURE; }
		std::uint64_t value(0);
		if (opt.ld_window) {
			if (!parse_count(opt.ld_window, value) || value < 1 || value > V2M_SITE_LD_MAX_WINDOW) { std::cerr << "ERROR: --ld-window must be a number of sites from 1 to " << V2M_SITE_LD_MAX_WINDOW << ", got \"" << opt.ld_window << "\".\n"; return EXIT_FAILURE; }
			opt.ld_params.window_sites = std::uint32_t(value);
		}
		if (opt.ld_window_columns) {
			if (!parse_count(opt.ld_window_columns, value)) { std::cerr << "ERROR: --ld-window-columns must be a number of columns, got \"" << opt.ld_window_columns << "\".\n"; return EXIT_FAILURE; }
			opt.ld_params.window_columns = value;
		}
		if (opt.ld_min_count) {
			if (!parse_count(opt.ld_min_count, value) || value < 1 || value > 0xFFFFFFFFull) { std::cerr << "ERROR: --ld-min-count must be a count of at least 1, got \"" << opt.ld_min_count << "\".\n"; return EXIT_FAILURE; }
			opt.ld_params.min_allele_count = std::uint32_t(value);
		}
		if (opt.ld_min_r2 && !vh::parse_decimal_fraction(opt.ld_min_r2, opt.ld_params.min_r2_num, opt.ld_params.min_r2_den)) {
			std::cerr << "ERROR: --ld-min-r2 must be a decimal number from 0 to 1 with at most 6 decimals, got \"" << opt.ld_min_r2 << "\".\n";
			return EXIT_FAILURE;
		}
	}
	if (opt.region && !parse_region(opt.region, opt.region_start, opt.region_end)) {
		std::cerr << "ERROR: --region must be START-END with 1 <= START <= END (1-based, inclusive), got \"" << opt.region << "\".\n";
		return EXIT_FAILURE;
	}

	try {
		// BGZF inputs are recognised and their framing checked before any device is needed: gzip that is not BGZF and broken
		// framing end the run here, with or without a GPU.
		std::unique_ptr<vh::input_file> ref_input(new vh::input_file(opt.input_reference)), variants_input;
		if (opt.input_variants) variants_input.reset(new vh::input_file(opt.input_variants));
		for (auto const *in : {ref_input.get(), variants_input.get()}) {
			if (!in || !in->bgzf()) continue;
			char const *const path(in == ref_input.get() ? opt.input_reference : opt.input_variants);
			if (!in->ends_with_eof())
				std::cerr << "WARNING: " << path << " does not end with the BGZF EOF member; the file may be truncated.\n";
		}
		auto const report_inflate([&](vh::input_file const &in, char const *path) {
			if (opt.verbose)
				std::cerr << "BGZF input " << path << ": " << in.members() << " members, " << in.bytes() << " bytes, inflated on the GPU in "
					<< in.inflate_seconds() << " s.\n";
		});

		// The GPU contexts come up on a second thread (HIP runtime start-up and stream creation: 0.2 s) while this one reads the
		// reference and the graph; without a usable MI355X the run still fails, loudly, at the first use below.
		auto contexts_coming(std::async(std::launch::async, [&opt] {
			std::vector<std::unique_ptr<vh::gpu_context>> contexts;
			for (int const device : opt.devices) contexts.emplace_back(new vh::gpu_context(device));
			return contexts;
		}));
		std::vector<std::unique_ptr<vh::gpu_context>> contexts;
		auto const first_gpu([&]() -> vh::gpu_context & {
			if (contexts.empty()) contexts = contexts_coming.get();
			return *contexts.front();
		});

		vh::sequence_type ref_seq;
		std::cerr << "Reading the reference sequence..." << std::flush;
		bool ref_read(false);
		if (ref_input->bgzf()) {
			std::string_view const text(ref_input->inflate(first_gpu()));
			report_inflate(*ref_input, opt.input_reference);
			ref_read = vh::read_single_fasta_sequence(text, ref_seq, opt.reference_sequence);
		} else ref_read = vh::read_single_fasta_sequence(opt.input_reference, ref_seq, opt.reference_sequence);
		ref_input.reset();
		if (!ref_read) {
			std::cerr << " ERROR: Unable to read the reference sequence.\n";
			return EXIT_FAILURE;
		}
		std::cerr << " Done. Reference length is " << ref_seq.size() << ".\n";
		if (opt.region && opt.region_end > ref_seq.size()) {
			std::cerr << "ERROR: --region end " << opt.region_end << " is past the end of the reference sequence (" << ref_seq.size() << ").\n";
			return EXIT_FAILURE;
		}
		std::vector<bed_region> bed_regions;
		if (opt.regions_file) {
			std::uint64_t skipped(0);
			std::string const problem(read_regions_file(opt.regions_file, opt.chromosome, ref_seq.size(), bed_regions, skipped));
			if (!problem.empty()) { std::cerr << "ERROR: --regions-file: " << problem << ".\n"; return EXIT_FAILURE; }
			if (opt.verbose) std::cerr << "Regions file " << opt.regions_file << ": " << bed_regions.size() << " regions taken, " << skipped << " lines of other chromosomes skipped.\n";
		}
		// A missing or unusable GPU, or a bad --device, should end the run here, before the variants are parsed, not minutes later.
		// HIP's start-up takes 0.2 s whether it ends in a context or in an error, so after a reference of any size (100 Mb: 0.07 s
		// + 30 ms of grace here; a genome: seconds) the outcome is usually in; when it is not, waiting for it would only take the
		// overlap with the graph's loading away (0.1 s at config 3), and the first use reports the failure all the same.
		if (contexts.empty() && std::future_status::ready == contexts_coming.wait_for(std::chrono::milliseconds(30))) (void) first_gpu();   // (a BGZF reference took them already)

		vh::variant_graph graph;
		if (opt.input_graph) {                                  // main.cc:392-401
			std::cerr << "Loading the variant graph from " << opt.input_graph << "..." << std::flush;
			vh::read_graph(opt.input_graph, graph);
			std::cerr << " Done.\n";
		} else {
			sample_set included, excluded;
			build_delegate delegate;
			delegate.chromosome = opt.chromosome;
			delegate.mismatch_is_error = opt.ref_mismatch_error;
			if (opt.include_samples) { included = read_sample_list(opt.include_samples, opt.chromosome); delegate.included = &included; }
			if (opt.exclude_samples) { excluded = read_sample_list(opt.exclude_samples, opt.chromosome); delegate.excluded = &excluded; }
			std::ofstream overlaps_os;
			if (opt.output_overlaps) {
				overlaps_os.open(opt.output_overlaps);
				delegate.overlaps = &overlaps_os;
				delegate.is_tsv = true;
			}
			std::cerr << "Building the variant graph...\n";
			vh::build_graph_statistics stats;
			bool scanned(false);
			if (opt.gpu_parse) {
				// the compressed members (or the plain text) go to the GPU slice by slice; what comes back is line records, the records'
				// first nine columns and the path bits
				vh::scan_statistics scan;
				try {
					if (variants_input->bgzf())
						vh::build_variant_graph_gpu_parsed(first_gpu(), opt.input_variants, variants_input->compressed(), variants_input->bytes(), ref_seq, opt.chromosome, graph, stats, delegate, &scan, 64);
					else {
						vh::mapped_file const file(opt.input_variants);
						vh::build_variant_graph_gpu_parsed(first_gpu(), opt.input_variants, std::string_view(file.data, file.size), file.size, ref_seq, opt.chromosome, graph, stats, delegate, &scan, 64);
					}
					scanned = true;
					if (opt.verbose) std::cerr << "GPU parse of " << opt.input_variants << ": " << scan.lines << " lines scanned, " << scan.declined << " declined (parsed from their text).\n";
				} catch (vh::gpu_error const &e) {
					// nothing has been merged when the layout is refused; a line longer than a slice may turn up later, and the records
					// before it have been reported to the delegate by then
					if (V2M_ERR_UNSUPPORTED != e.code || stats.handled_variants) throw;
					if (opt.verbose) std::cerr << "GPU parse not supported for this input (" << e.what() << "); parsing the text on the host.\n";
					stats = vh::build_graph_statistics{};
				}
			}
			if (!scanned) {
				if (variants_input->bgzf()) {
					std::string_view const text(variants_input->inflate(first_gpu()));
					report_inflate(*variants_input, opt.input_variants);
					vh::build_variant_graph(ref_seq, text, opt.chromosome, graph, stats, delegate, 0, 64);
				} else
					vh::build_variant_graph(ref_seq, opt.input_variants, opt.chromosome, graph, stats, delegate, 0, 64);   // the reference's padding (variant_graph.cc:277,449)
			}
			variants_input.reset();                             // (the decompressed text)
			// variant_graph.cc:453 (the transpose) happens on the GPU(s) below; the transposed matrix only comes back to the host
			// when something on the host reads it: the founder search and the graph checkpoint.
			if (opt.founder_mode || opt.output_graph) vh::transpose_paths(first_gpu(), graph);
			std::cerr << "Done. Handled variants: " << stats.handled_variants << " Chromosome ID mismatches: " << stats.chr_id_mismatches << '\n';
			if (0 == stats.handled_variants) std::cerr << "WARNING: no variants matched the chromosome identifier \"" << opt.chromosome << "\".\n";
		}

		if (opt.output_tree && opt.haplotypes && graph.total_chromosome_copies() + (opt.omit_reference ? 0 : 1) < 3) {
			std::cerr << "ERROR: --output-tree needs at least three sequences (got " << graph.total_chromosome_copies() + (opt.omit_reference ? 0 : 1) << ").\n";
			return EXIT_FAILURE;
		}

		if (opt.haplotypes && !opt.diversity_group_of.empty()) {
			// the names --output-distances gives the rows (output.cc: haplotype_output::rows_for), known before a device is opened
			std::set<std::string> known;
			std::string const prefix(opt.dst_chromosome ? std::string(opt.dst_chromosome) + '.' : std::string());
			if (!opt.omit_reference) known.insert(prefix + "REF");
			for (std::size_t s(0); s < graph.sample_names.size(); ++s)
				for (vh::u32 c(0); c < graph.sample_ploidy(s); ++c) known.insert(prefix + graph.sample_names[s] + '.' + std::to_string(1 + c));
			for (auto const &[id, group] : opt.diversity_group_of)
				if (!known.count(id)) { std::cerr << "ERROR: " << opt.diversity_groups << ": \"" << id << "\" names no output sequence.\n"; return EXIT_FAILURE; }
		}

		if (opt.output_graph) {                                 // main.cc:418-426
			std::cerr << "Outputting the variant graph..." << std::flush;
			vh::write_graph(graph, opt.output_graph);
			std::cerr << " Done.\n";
		}

		if (opt.graph_statistics) {   // main.cc:428-435
			std::cout << "Nodes:        " << graph.node_count() << '\n';
			std::cout << "ALT edges:    " << graph.edge_count() << '\n';
			std::cout << "Total ploidy: " << graph.total_chromosome_copies() << '\n';
		}

		// Graph and reference are replicated on every GPU; the path matrix is not.  With several GPUs, GPU k
		// receives the bits of its own chromosome copies only, transposes them itself and splices the rows of those copies:
		//  - an aligned A2M file as the only output: contiguous blocks of copies, every GPU's thread writes its rows at their
		//    final file offsets (all aligned rows have the same length);
		//  - every output that has to leave in row order (pipes, unaligned A2M, one file per sequence): the copies dealt
		//    round-robin in blocks of 8, so that every GPU always has rows that are due soon, handed to the writer in turns.
		// Founder rows read copies all over the matrix: every GPU then holds all of it.
		vh::gpu_context &gpu(first_gpu());
		std::vector<vh::gpu_context *> all_gpus;
		for (auto &g : contexts) all_gpus.push_back(g.get());
		bool const several(opt.haplotypes && all_gpus.size() > 1);
		bool const sharded(several && opt.output_sequences_a2m && !opt.pipe && !opt.unaligned && !opt.output_sequences_separate && !opt.bgzf);   // BGZF sizes are not known up front
		bool const interleaved(several && !sharded);
		vh::copy_interleave const deal{8, vh::u32(all_gpus.size())};
		std::vector<vh::copy_shard> shards;
		std::future<void> founder_graph_uploaded;
		if (opt.founder_mode) {
			// The first context gets the graph with its (transposed) path matrix now: the cut search walks its chunks there
			// (v2m_pbwt_cut_trials).  The other contexts' uploads and the output path's buffers are set up while the search runs.
			vh::upload_graph(gpu, ref_seq, graph, true);
			founder_graph_uploaded = std::async(std::launch::async, [&] {
				for (std::size_t k(1); k < all_gpus.size(); ++k) vh::upload_graph(*all_gpus[k], ref_seq, graph, true);
				for (std::size_t k(1); k < all_gpus.size(); ++k) vh::warm_up_sink(*all_gpus[k], opt.unaligned);
			});
		}
		if (!opt.founder_mode) {
			// every context's graph and matrix share go up on that context's own thread (one PCIe link each)
			std::vector<std::exception_ptr> upload_errors(all_gpus.size());
			std::vector<std::thread> uploaders;
			for (std::size_t k(0); k < all_gpus.size(); ++k) {
				vh::copy_shard const shard(sharded
					? vh::shard_copies(graph.total_chromosome_copies(), vh::u32(all_gpus.size()), vh::u32(k))
					: vh::copy_shard{0, graph.paths_by_edge_and_chrom_copy.rows});
				if (sharded) shards.push_back(shard);
				if (opt.verbose && sharded) std::cerr << "GPU context " << k << " (device " << opt.devices[k] << "): chromosome copies [" << shard.first << ", " << shard.end << ")\n";
				if (opt.verbose && interleaved) std::cerr << "GPU context " << k << " (device " << opt.devices[k] << "): chromosome copies " << deal.block * k << " + " << deal.block * deal.world << " j + [0, " << deal.block << "), j = 0, 1, ...\n";
				uploaders.emplace_back([&, k, shard] {
					try {
						vh::upload_graph(*all_gpus[k], ref_seq, graph, false);
						if (interleaved) vh::upload_path_blocks(*all_gpus[k], graph, deal, vh::u32(k));
						else vh::upload_path_slice(*all_gpus[k], graph, shard);
					} catch (...) {
						upload_errors[k] = std::current_exception();
					}
				});
			}
			for (auto &u : uploaders) u.join();
			for (auto const &e : upload_errors) if (e) std::rethrow_exception(e);
		}
		progress_delegate delegate;
		delegate.verbose = opt.verbose;
		// --region: every context produces the window of columns of reference range [START - 1, END) (include/v2m_hip.h, column windows);
		// the founder search above has run over the whole chromosome.  Set after the uploads, which reset it.
		auto const apply_region([&] {
			if (!opt.region) return;
			auto const w(vh::columns_of_reference_range(graph, ref_seq.size(), opt.region_start - 1, opt.region_end));
			if (opt.verbose) std::cerr << "Region " << opt.region_start << '-' << opt.region_end << ": alignment columns [" << w.begin << ", " << w.end << ") of " << graph.aligned_length() << ".\n";
			for (auto *g : all_gpus) g->check(v2m_set_column_window(g->get(), w.begin, w.end));
		});
		auto const do_output([&](vh::output &output) {   // main.cc:456-473
			if (opt.regions_file) {
				std::vector<vh::output_region> regions;
				for (auto const &r : bed_regions) {
					auto const w(vh::columns_of_reference_range(graph, ref_seq.size(), r.start, r.end));
					regions.push_back({r.name, w.begin, w.end});
				}
				std::size_t const per_pass(regions_per_pass(opt.distinct ? 2 : 1));
				std::cerr << "Outputting " << regions.size() << " regions, " << (opt.distinct ? "the distinct sequences of each in one file..." : "one file each...") << std::flush;
				if (opt.verbose) std::cerr << " (" << (regions.size() + per_pass - 1) / per_pass << " passes of at most " << per_pass << " regions)" << std::flush;
				output.output_regions(graph, regions, per_pass, opt.distinct, opt.verbose);
				std::cerr << " Done.\n";
			}
			if (opt.output_sequences_a2m) {
				std::cerr << "Outputting sequences as A2M...\n";
				output.output_a2m(graph, opt.output_sequences_a2m);
				std::cerr << "Done.\n";
			}
			if (opt.output_sequences_separate) {
				std::cerr << "Outputting sequences one by one..." << std::flush;
				output.output_separate(graph, !opt.separate_plain);
				std::cerr << " Done.\n";
			}
			if (opt.output_chain && opt.output_paf) {   // one pass over the rows, with the split; the chains from the ops folded back
				std::cerr << "Outputting chains and PAF..." << std::flush;
				output.output_chain_and_paf(graph, opt.output_chain, opt.output_paf);
				std::cerr << " Done.\n";
			} else if (opt.output_chain) {
				std::cerr << "Outputting chains..." << std::flush;
				output.output_chain(graph, opt.output_chain);
				std::cerr << " Done.\n";
			} else if (opt.output_paf) {
				std::cerr << "Outputting PAF..." << std::flush;
				output.output_paf(graph, opt.output_paf);
				std::cerr << " Done.\n";
			}
			if (opt.output_column_counts) {
				std::cerr << "Outputting column counts..." << std::flush;
				output.output_column_counts(graph, opt.output_column_counts, opt.all_columns, opt.verbose);
				std::cerr << " Done.\n";
			}
			if (opt.output_distances) {
				std::cerr << "Outputting distances..." << std::flush;
				output.output_distances(graph, opt.output_distances, opt.acgt_only, opt.verbose);
				std::cerr << " Done.\n";
			}
			if (opt.output_variable_sites) {
				std::cerr << "Outputting variable sites..." << std::flush;
				output.output_variable_sites(graph, opt.output_variable_sites, opt.snp_sites, opt.output_site_positions, opt.verbose);
				std::cerr << " Done.\n";
			}
			if (opt.output_ld) {
				std::cerr << "Outputting site LD..." << std::flush;
				output.output_ld(graph, opt.output_ld, opt.ld_params, opt.verbose);
				std::cerr << " Done.\n";
			}
			if (opt.output_diversity || opt.diversity_sfs || opt.output_divergence) {
				std::cerr << "Outputting the window diversity..." << std::flush;
				vh::output::diversity_params params;
				params.window = opt.diversity_window_bp;
				params.step = opt.diversity_step_bp;
				params.ref_len = ref_seq.size();
				params.ref_begin = opt.region ? opt.region_start - 1 : 0;
				params.ref_end = opt.region ? opt.region_end : ref_seq.size();
				params.groups = opt.diversity_group_of;
				output.output_diversity(graph, params, opt.output_diversity, opt.diversity_sfs, opt.output_divergence, opt.verbose);
				std::cerr << " Done.\n";
			}
			if (opt.output_tree) {
				std::cerr << "Outputting the tree..." << std::flush;
				output.output_tree(graph, opt.output_tree, opt.tree_acgt_only, opt.verbose, opt.tree_replicates, opt.tree_seed_value, opt.output_tree_replicates);
				std::cerr << " Done.\n";
				if (opt.output_tree_parsimony || opt.output_tree_mutations || opt.output_tree_sites) {
					std::cerr << "Outputting the parsimony on the tree..." << std::flush;
					output.output_tree_parsimony(graph, opt.output_tree_parsimony, opt.output_tree_mutations, opt.output_tree_sites, opt.verbose);
					std::cerr << " Done.\n";
				}
			}
		});

		if (opt.haplotypes) {
			vh::haplotype_output output(gpu, opt.pipe, opt.dst_chromosome, !opt.omit_reference, opt.unaligned, delegate);
			for (std::size_t k(1); k < all_gpus.size(); ++k) output.add_gpu(*all_gpus[k]);
			if (sharded) output.set_copy_shards(shards);
			if (interleaved) output.set_copy_interleave(deal);
			output.set_bgzf(opt.bgzf);
			apply_region();
			do_output(output);
		} else {                                            // main.cc:487-550
			vh::founder_sequence_greedy_output output(gpu, opt.pipe, opt.dst_chromosome, !opt.omit_reference, opt.unaligned, delegate);
			for (std::size_t k(1); k < all_gpus.size(); ++k) output.add_gpu(*all_gpus[k]);
			std::vector<vh::u64> cuts;
			vh::u32 score(0);
			vh::gpu_founder_walker walker(gpu);   // the chunk walks of both searches run on the first context (v2m_pbwt_cut_trials / _records)
			vh::u64 cut_min_distance(vh::u64(opt.minimum_distance));
			if (opt.input_cut_positions) {                  // main.cc:499-500
				auto loaded(vh::read_cut_positions(opt.input_cut_positions));
				cuts = std::move(loaded.cut_positions);
				score = loaded.score;
				cut_min_distance = loaded.min_distance;
			} else {
				std::cerr << "Optimising cut positions...\n";
				score = vh::find_cut_positions(graph, vh::u64(opt.minimum_distance), cuts, 0, &walker);
				if (opt.verbose) std::cerr << "Cut search: " << walker.chunks_walked << " chunks walked on the GPU, " << walker.chunks_left << " on the host.\n";
				if (vh::kCutPositionScoreMax == score) { std::cerr << "ERROR: Unable to optimise cut positions.\n"; return EXIT_FAILURE; }
				if (opt.verbose) {
					std::cout << "Cut positions:";
					for (auto const cp : cuts) std::cout << ' ' << cp;
					std::cout << '\n';
				}
			}
			std::cout << "Maximum segmentation height: " << (1 + vh::u64(score)) << '\n';   // main.cc:520
			if (opt.output_cut_positions)                   // main.cc:522-523
				vh::write_cut_positions({cuts, cut_min_distance, score}, opt.output_cut_positions);
			std::cerr << "Finding matchings in the variant graph...\n";
			std::vector<vh::u32> assigned;
			// the first context is idle once the matching's chunk walks are back: its output buffers (a gigabyte of pinned memory,
			// 0.15 s) are set up on another thread while the greedy assignment runs here
			std::future<void> first_sink_warm;
			walker.on_last_walk = [&] { first_sink_warm = std::async(std::launch::async, [&] { vh::warm_up_sink(gpu, opt.unaligned); }); };
			if (!vh::find_matchings(graph, cuts, vh::u32(opt.founder_sequences), opt.keep_ref_edges, assigned, 0, &walker)) { std::cerr << "ERROR: Unable to find matchings.\n"; return EXIT_FAILURE; }
			if (opt.verbose) {                              // main.cc:534-545
				std::cout << "Matchings:\n";
				std::size_t const rows(cuts.size() - 1);
				for (long col(0); col < opt.founder_sequences; ++col) {
					std::cout << col << ':';
					for (std::size_t r(0); r < rows; ++r) std::cout << '\t' << assigned[col * rows + r];
					std::cout << '\n';
				}
			}
			output.set_cut_positions(std::move(cuts));
			output.set_assigned_samples(std::move(assigned), vh::u32(opt.founder_sequences));
			output.set_bgzf(opt.bgzf);
			founder_graph_uploaded.get();
			if (first_sink_warm.valid()) first_sink_warm.get(); else vh::warm_up_sink(gpu, opt.unaligned);
			apply_region();
			do_output(output);
		}
	} catch (vh::gpu_error const &e) {
		std::cerr << "ERROR (GPU path, code " << e.code << "): " << e.what() << '\n';
		return EXIT_FAILURE;
	} catch (std::exception const &e) {
		std::cerr << "ERROR: " << e.what() << '\n';
		return EXIT_FAILURE;
	}
	return EXIT_SUCCESS;
}
