// readers.hh -- plain-text input for the host driver: single-sequence FASTA and VCF -> variant graph.
//
// These stand in for the libbio readers the reference uses (lb::read_single_fasta_sequence at
// vcf2multialign/main.cc:381, vcf::reader at libvcf2multialign/variant_graph.cc:133-146,181); libbio is an
// absent submodule, so only the behaviour visible at those call sites is reproduced.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

#include <functional>
#include <stdexcept>

#include "../../../include/v2m_hip.h"
#include "variant_graph.hh"

namespace v2m::host {

typedef std::vector<char> sequence_type;   // variant_graph.hh:33

// First sequence of the file, or the one whose identifier (text after '>' up to the first blank) equals seq_id.
bool read_single_fasta_sequence(char const *path, sequence_type &seq, char const *seq_id = nullptr);
// The same over FASTA text already in memory (a decompressed .fa.gz: gpu_path.hh, input_file).
bool read_single_fasta_sequence(std::string_view text, sequence_type &seq, char const *seq_id = nullptr);

// Read-only mapping of a whole file (the reference maps the VCF too: vcf::mmap_input, variant_graph.cc:133-134).  Throws
// std::runtime_error when the file cannot be opened, stat'ed or mapped.
struct mapped_file {
	char const *data{};
	std::size_t size{};
	int fd{-1};
	explicit mapped_file(char const *path);
	~mapped_file();
	mapped_file(mapped_file const &) = delete;
	mapped_file &operator=(mapped_file const &) = delete;
};

// variant_graph.hh:138-158
struct build_graph_delegate {
	virtual ~build_graph_delegate() {}
	virtual bool should_include(std::string_view sample_name, u32 chrom_copy_idx) const = 0;
	virtual void report_overlapping_alternative(
		u64 lineno, u64 ref_pos, std::string_view var_id, std::string_view sample_name, u32 chrom_copy_idx, u32 gt) = 0;
	// return false to stop building
	virtual bool ref_column_mismatch(u64 var_idx, u64 ref_pos, std::string_view ref_in_vcf, std::string_view expected) = 0;
};

// variant_graph.hh:167-171
struct build_graph_statistics {
	u64 handled_variants{};
	u64 chr_id_mismatches{};
};

// build_variant_graph (variant_graph.cc:108-454) up to, but not including, the final transpose at :453:
// paths_by_edge_and_chrom_copy is filled, paths_by_chrom_copy_and_edge is left for the GPU
// (gpu_path.hh: transpose_paths).  Throws std::runtime_error on malformed input.
//
// The reference parses and builds on one thread.  Here the genotype text -- 5 * 10^9 fields at config 3 -- is
// parsed by `threads` workers over 8-MB chunks of whole lines into sparse (copy, allele) lists, and one thread
// merges the chunks in file order through graph_builder, so the graph and the delegate calls are exactly those
// of a sequential pass.  threads == 0: one per hardware thread, at most 16.  path_alignment: see graph_builder.
void build_variant_graph(
	sequence_type const &ref_seq, char const *variants_path, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, unsigned threads = 0, u64 path_alignment = 64);
// The same over VCF text already in memory (a decompressed .vcf.gz: gpu_path.hh, input_file); the path version maps the file and calls this.
void build_variant_graph(
	sequence_type const &ref_seq, std::string_view variants_text, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, unsigned threads = 0, u64 path_alignment = 64);

// ---- the scanned path: the graph from line records, heads and bit columns instead of text (include/v2m_hip.h, "VCF scan") ----

// A scan of the whole VCF for `chr_id`: v2m_vcf_scan on a GPU context (gpu_path.hh: build_variant_graph_gpu_parsed), or scan_lines_host below.
// Returns a V2M_* code.
typedef std::function<int(char const *chr_id, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user)> line_scanner;

struct scan_statistics {
	u64 lines{};       // lines scanned
	u64 declined{};    // of them of kind 3: parsed from their text by the host
};

// The scanner returned a code other than V2M_OK and no callback had failed (V2M_ERR_UNSUPPORTED: the caller uses the text path).
struct scan_failed : std::runtime_error {
	int code;
	explicit scan_failed(int code_) : std::runtime_error("the VCF scan failed with code " + std::to_string(code_)), code(code_) {}
};

// The rule of v2m_vcf_scan in plain C++, over text in memory: the same chunks from the same text (a slice = the line the
// previous slice ended in, carried over, plus as many new bytes as slice_bytes still holds, its whole lines delivered; 0 = 64 MiB; a line
// that no slice holds is V2M_ERR_UNSUPPORTED), byte for byte what the kernels give for the same lines.  It is what the GPU
// tests compare the kernels with, and it makes the assembler testable without a GPU.
int scan_lines_host(std::string_view text, char const *wanted_chr, std::size_t slice_bytes, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user);

// build_variant_graph through a scanner: the layout callback runs the first-record code on the line it is given, the chunk callback fills
// a chunk of the merge stage from the scanned lines (lines of kind 2: the head through the text parser's head part, the bit columns mapped
// to edge columns; kind 3: the text parser on the whole line, with its errors; kinds 0 and 1: counted) and merges it, on the scanner's
// thread (a delegate that stops the build at a REF mismatch ends the scan there; the scan statistics then cover the lines up to that
// chunk).  The graph, the statistics, the delegate calls and the errors are those of build_variant_graph on the same text.  Throws
// scan_failed when the scanner itself fails; expected_text_bytes: the size of the text (a hint for the path matrix's allocation).
void build_variant_graph_scanned(
	sequence_type const &ref_seq, line_scanner const &scanner, u64 expected_text_bytes, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, scan_statistics *scan_stats = nullptr, u64 path_alignment = 64);

} // namespace v2m::host
