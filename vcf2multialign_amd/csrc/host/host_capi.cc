// host_capi.cc -- C API over the host-side graph builder so that the Python tests can compare it with the
// oracle's builder array by array (no GPU involved: the transpose is not part of the host builder).

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "founder.hh"
#include "gpu_path.hh"
#include "graph_file.hh"
#include "output.hh"
#include "readers.hh"

namespace vh = v2m::host;

namespace {

struct recorded_overlap { vh::u64 lineno, ref_pos; std::string var_id, sample; vh::u32 copy, gt; };

struct host_graph {
	vh::variant_graph graph;
	vh::sequence_type ref;
	vh::build_graph_statistics stats;
	std::vector<recorded_overlap> overlaps;
	std::string sample_blob;
	vh::scan_statistics scan;      // the scanned builds: lines scanned, lines declined
};

struct recording_delegate final : vh::build_graph_delegate {
	host_graph *hg{};
	std::string excluded_sample;   // optional: exclude every copy of this sample
	int excluded_copy{-1};         // or only this copy
	bool should_include(std::string_view sample_name, vh::u32 copy) const override
	{
		if (excluded_sample.empty() || sample_name != excluded_sample) return true;
		return excluded_copy >= 0 && int(copy) != excluded_copy;
	}
	void report_overlapping_alternative(vh::u64 lineno, vh::u64 ref_pos, std::string_view var_id, std::string_view sample_name, vh::u32 copy, vh::u32 gt) override
	{
		hg->overlaps.push_back({lineno, ref_pos, std::string(var_id), std::string(sample_name), copy, gt});
	}
	bool stop_at_mismatch{};       // what the reference's delegate may also answer: stop parsing here (variant_graph.cc:312-313)
	bool ref_column_mismatch(vh::u64, vh::u64, std::string_view, std::string_view) override
	{
		if (stop_at_mismatch) return false;
		throw std::runtime_error("REF column mismatch");
	}
};

bool g_stop_at_mismatch(false);

// The host graph of the two files.  gpu == NULL: both through the path readers.  Otherwise either file may be BGZF (gpu_path.hh:
// input_file), inflated on that context; plain files still go through the path readers.
// scanner: 0 = the text path; 1 = the VCF through v2m_vcf_scan on `gpu` (BGZF or plain, never inflated to the host); 2 = through scan_lines_host
// (plain text only, no GPU).
host_graph *build_host_graph(vh::gpu_context *gpu, char const *fasta, char const *seq_id, char const *vcf, char const *chr, char const *exclude_sample,
	int exclude_copy, unsigned threads, char *err, size_t errlen, int scanner = 0)
{
	auto *hg(new host_graph);
	try {
		{
			std::unique_ptr<vh::input_file> in(gpu ? new vh::input_file(fasta) : nullptr);
			bool const ok(in && in->bgzf() ? vh::read_single_fasta_sequence(in->inflate(*gpu), hg->ref, seq_id) : vh::read_single_fasta_sequence(fasta, hg->ref, seq_id));
			if (!ok) throw std::runtime_error("unable to read the reference sequence");
		}
		recording_delegate d;
		d.hg = hg;
		if (exclude_sample) { d.excluded_sample = exclude_sample; d.excluded_copy = exclude_copy; }
		d.stop_at_mismatch = g_stop_at_mismatch;
		std::unique_ptr<vh::input_file> in(gpu ? new vh::input_file(vcf) : nullptr);
		if (1 == scanner) {
			if (!gpu) throw std::runtime_error("the GPU scanner needs a GPU context");
			if (in->bgzf()) vh::build_variant_graph_gpu_parsed(*gpu, vcf, in->compressed(), in->bytes(), hg->ref, chr, hg->graph, hg->stats, d, &hg->scan);
			else {
				vh::mapped_file const file(vcf);
				vh::build_variant_graph_gpu_parsed(*gpu, vcf, std::string_view(file.data, file.size), file.size, hg->ref, chr, hg->graph, hg->stats, d, &hg->scan);
			}
		} else if (2 == scanner) {
			vh::mapped_file const file(vcf);
			std::string_view const text(file.data, file.size);
			std::size_t slice(0);
			if (char const *const e = std::getenv("V2M_RING_SLOT_BYTES")) if (*e) slice = std::strtoull(e, nullptr, 10);   // test knob, as for v2m_vcf_scan
			vh::line_scanner const host_scanner([&](char const *c, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user) {
				return vh::scan_lines_host(text, c, slice, layout, chunk, user);
			});
			vh::build_variant_graph_scanned(hg->ref, host_scanner, text.size(), chr, hg->graph, hg->stats, d, &hg->scan);
		}
		else if (in && in->bgzf()) vh::build_variant_graph(hg->ref, in->inflate(*gpu), chr, hg->graph, hg->stats, d, threads);
		else vh::build_variant_graph(hg->ref, vcf, chr, hg->graph, hg->stats, d, threads);
		for (auto const &s : hg->graph.sample_names) { hg->sample_blob += s; hg->sample_blob.push_back('\0'); }
		return hg;
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		delete hg;
		return nullptr;
	}
}

} // namespace

extern "C" {

void *v2mh_build_variant_graph(char const *fasta, char const *seq_id, char const *vcf, char const *chr, char const *exclude_sample, int exclude_copy, unsigned threads, char *err, size_t errlen)
{
	return build_host_graph(nullptr, fasta, seq_id, vcf, chr, exclude_sample, exclude_copy, threads, err, errlen);
}

// v2mh_build_variant_graph with BGZF input allowed for either file (gpu_path.hh: input_file), inflated on the GPU of `ctx` (a v2m_ctx the
// caller owns); plain files are read exactly as v2mh_build_variant_graph reads them.
void *v2mh_build_variant_graph_gpu(void *ctx, char const *fasta, char const *seq_id, char const *vcf, char const *chr, char const *exclude_sample, int exclude_copy,
	unsigned threads, char *err, size_t errlen)
{
	if (!ctx) {
		if (err && errlen) { std::strncpy(err, "v2mh_build_variant_graph_gpu needs a GPU context", errlen - 1); err[errlen - 1] = 0; }
		return nullptr;
	}
	vh::gpu_context gpu(static_cast<v2m_ctx *>(ctx), vh::gpu_context::borrowed{});
	return build_host_graph(&gpu, fasta, seq_id, vcf, chr, exclude_sample, exclude_copy, threads, err, errlen);
}

// The same with the VCF's genotype columns scanned instead of parsed from text (readers.hh: build_variant_graph_scanned).  scanner = 1:
// v2m_vcf_scan on `ctx` (the VCF BGZF or plain; the FASTA as for v2mh_build_variant_graph_gpu); scanner = 2: scan_lines_host, plain files, ctx
// may be NULL.  `threads` is accepted for symmetry: the scanned build assembles and merges on the scanner's thread.
void *v2mh_build_variant_graph_scanned(void *ctx, char const *fasta, char const *seq_id, char const *vcf, char const *chr, char const *exclude_sample, int exclude_copy,
	unsigned threads, char *err, size_t errlen, int scanner)
{
	if (1 != scanner && 2 != scanner) {
		if (err && errlen) { std::strncpy(err, "v2mh_build_variant_graph_scanned: scanner must be 1 (GPU) or 2 (host)", errlen - 1); err[errlen - 1] = 0; }
		return nullptr;
	}
	if (!ctx) {
		if (1 == scanner) { if (err && errlen) { std::strncpy(err, "v2mh_build_variant_graph_scanned needs a GPU context for the GPU scanner", errlen - 1); err[errlen - 1] = 0; } return nullptr; }
		return build_host_graph(nullptr, fasta, seq_id, vcf, chr, exclude_sample, exclude_copy, threads, err, errlen, scanner);
	}
	vh::gpu_context gpu(static_cast<v2m_ctx *>(ctx), vh::gpu_context::borrowed{});
	return build_host_graph(&gpu, fasta, seq_id, vcf, chr, exclude_sample, exclude_copy, threads, err, errlen, scanner);
}

// Lines the scanned build scanned, and those of them it declined (kind 3: parsed from their text).
void v2mh_scan_statistics(void *h, uint64_t *lines, uint64_t *declined)
{
	*lines = static_cast<host_graph *>(h)->scan.lines;
	*declined = static_cast<host_graph *>(h)->scan.declined;
}

// scan_lines_host (readers.hh) over `n` bytes of text, for tests and tools: the callbacks are v2m_vcf_scan's.
int v2mh_scan_lines_host(char const *text, uint64_t n, char const *wanted_chr, uint64_t slice_bytes, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user)
{
	try { return vh::scan_lines_host(std::string_view(text, n), wanted_chr, slice_bytes, layout, chunk, user); }
	catch (std::exception const &) { return V2M_ERR_INVALID_ARGUMENT; }
}

// A host graph from flat arrays (e.g. a synthetic dataset whose genotype matrix was generated on the GPU):
// paths_by_edge_and_chrom_copy words are column-major, rows = path_rows copies (multiple of 64), cols = path_cols edges.
void *v2mh_graph_from_arrays(
	uint64_t n_nodes, uint64_t n_edges, uint64_t const *ref_pos, uint64_t const *aln_pos, uint64_t const *targets, uint64_t const *csum,
	uint64_t const *label_offsets, char const *label_bytes, uint64_t const *paths_by_edge_and_chrom_copy, uint64_t path_rows, uint64_t path_cols,
	uint32_t n_samples, uint32_t ploidy)
{
	auto *hg(new host_graph);
	auto &g(hg->graph);
	g.reference_positions.assign(ref_pos, ref_pos + n_nodes);
	g.aligned_positions.assign(aln_pos, aln_pos + n_nodes);
	g.alt_edge_targets.assign(targets, targets + n_edges);
	g.alt_edge_count_csum.assign(csum, csum + n_nodes + 1);
	g.alt_edge_label_offsets.assign(label_offsets, label_offsets + n_edges + 1);
	g.alt_edge_label_bytes.assign(label_bytes, label_bytes + label_offsets[n_edges]);
	g.paths_by_edge_and_chrom_copy = vh::bit_matrix(path_rows, path_cols);
	if (paths_by_edge_and_chrom_copy)
		std::copy(paths_by_edge_and_chrom_copy, paths_by_edge_and_chrom_copy + path_rows / 64 * path_cols, g.paths_by_edge_and_chrom_copy.words.begin());
	g.ploidy_csum.assign(1, 0);
	for (uint32_t s(0); s < n_samples; ++s) { g.sample_names.push_back("S" + std::to_string(s)); g.ploidy_csum.push_back(g.ploidy_csum.back() + ploidy); }
	for (auto const &s : g.sample_names) { hg->sample_blob += s; hg->sample_blob.push_back('\0'); }
	return hg;
}

void v2mh_free(void *h) { delete static_cast<host_graph *>(h); }

// How the next v2mh_build_variant_graph() calls answer a REF column mismatch: 0 = it is an error (default), 1 = stop parsing there.
void v2mh_set_stop_at_ref_mismatch(int stop) { g_stop_at_mismatch = 0 != stop; }

int v2mh_write_graph(void *h, char const *path, char *err, size_t errlen)
{
	try { vh::write_graph(static_cast<host_graph *>(h)->graph, path); return 0; }
	catch (std::exception const &e) { if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; } return 1; }
}

void *v2mh_read_graph(char const *path, char *err, size_t errlen)
{
	auto *hg(new host_graph);
	try {
		vh::read_graph(path, hg->graph);
		for (auto const &s : hg->graph.sample_names) { hg->sample_blob += s; hg->sample_blob.push_back('\0'); }
		return hg;
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		delete hg;
		return nullptr;
	}
}

#define HG(h) (*static_cast<host_graph *>(h))
uint64_t v2mh_node_count(void *h) { return HG(h).graph.node_count(); }
// The column window of the reference range [s, e) (gpu_path.hh: columns_of_reference_range); -1 for a range outside the reference.
int v2mh_columns_of_reference_range(void *h, uint64_t s, uint64_t e, uint64_t *col_begin, uint64_t *col_end)
{
	try {
		auto const w(vh::columns_of_reference_range(HG(h).graph, HG(h).ref.size(), s, e));
		*col_begin = w.begin;
		*col_end = w.end;
		return 0;
	} catch (std::invalid_argument const &) {
		return -1;
	}
}
uint64_t v2mh_edge_count(void *h) { return HG(h).graph.edge_count(); }
uint64_t v2mh_sample_count(void *h) { return HG(h).graph.sample_names.size(); }
uint64_t v2mh_ref_length(void *h) { return HG(h).ref.size(); }
char const *v2mh_reference(void *h) { return HG(h).ref.data(); }
uint64_t const *v2mh_reference_positions(void *h) { return HG(h).graph.reference_positions.data(); }
uint64_t const *v2mh_aligned_positions(void *h) { return HG(h).graph.aligned_positions.data(); }
uint64_t const *v2mh_alt_edge_targets(void *h) { return HG(h).graph.alt_edge_targets.data(); }
uint64_t const *v2mh_alt_edge_count_csum(void *h) { return HG(h).graph.alt_edge_count_csum.data(); }
uint64_t const *v2mh_label_offsets(void *h) { return HG(h).graph.alt_edge_label_offsets.data(); }
char const *v2mh_label_bytes(void *h) { return HG(h).graph.alt_edge_label_bytes.data(); }
char const *v2mh_sample_blob(void *h) { return HG(h).sample_blob.data(); }
uint64_t v2mh_sample_blob_size(void *h) { return HG(h).sample_blob.size(); }
uint32_t const *v2mh_ploidy_csum(void *h) { return HG(h).graph.ploidy_csum.data(); }
uint64_t v2mh_ploidy_csum_size(void *h) { return HG(h).graph.ploidy_csum.size(); }
uint64_t v2mh_handled_variants(void *h) { return HG(h).stats.handled_variants; }
uint64_t v2mh_chr_id_mismatches(void *h) { return HG(h).stats.chr_id_mismatches; }
uint64_t const *v2mh_paths_by_edge_and_chrom_copy(void *h, uint64_t *rows, uint64_t *cols)
{
	auto const &m(HG(h).graph.paths_by_edge_and_chrom_copy);
	*rows = m.rows; *cols = m.cols;
	return m.words.data();
}
uint64_t v2mh_overlap_count(void *h) { return HG(h).overlaps.size(); }
void v2mh_overlap_get(void *h, uint64_t i, uint64_t *lineno, uint64_t *ref_pos, char const **var_id, char const **sample, uint32_t *copy, uint32_t *gt)
{
	auto const &o(HG(h).overlaps[i]);
	*lineno = o.lineno; *ref_pos = o.ref_pos; *var_id = o.var_id.c_str(); *sample = o.sample.c_str(); *copy = o.copy; *gt = o.gt;
}

// find_cut_positions + find_matchings on a built graph.  cuts_out must hold node_count entries; assigned_out
// (cuts - 1) * founder_count entries (column-major).  Returns the number of cut positions, 0 if there is no
// solution; *score_out receives the segmentation score.
uint64_t v2mh_find_founders_mt(void *h, uint64_t min_distance, uint32_t founder_count, int keep_ref_edges,
	uint64_t *cuts_out, uint32_t *assigned_out, uint64_t assigned_capacity, uint32_t *score_out, unsigned threads)
{
	auto const &g(HG(h).graph);
	std::vector<vh::u64> cuts;
	vh::u32 const score(vh::find_cut_positions(g, min_distance, cuts, threads));
	if (score_out) *score_out = score;
	if (vh::kCutPositionScoreMax == score) return 0;
	std::vector<vh::u32> assigned;
	if (!vh::find_matchings(g, cuts, founder_count, 0 != keep_ref_edges, assigned, threads)) return 0;
	if (assigned.size() > assigned_capacity) return 0;
	std::copy(cuts.begin(), cuts.end(), cuts_out);
	std::copy(assigned.begin(), assigned.end(), assigned_out);
	return cuts.size();
}

// find_cut_positions with the chunk walks on the GPU context `ctx` (a v2m_ctx * that holds this graph with its path matrix).
// Returns the number of cut positions (0: no solution); cuts_out must hold node_count entries.
uint64_t v2mh_find_cut_positions_gpu(void *h, void *ctx, uint64_t min_distance, unsigned threads, uint64_t *cuts_out, uint32_t *score_out, uint64_t *chunks_walked_and_left, char *err, size_t errlen)
{
	try {
		vh::gpu_context gpu(static_cast<v2m_ctx *>(ctx), vh::gpu_context::borrowed{});
		vh::gpu_cut_trial_walker walker(gpu);
		std::vector<vh::u64> cuts;
		vh::u32 const score(vh::find_cut_positions(HG(h).graph, min_distance, cuts, threads, &walker));
		if (score_out) *score_out = score;
		if (chunks_walked_and_left) { chunks_walked_and_left[0] = walker.chunks_walked; chunks_walked_and_left[1] = walker.chunks_left; }
		if (vh::kCutPositionScoreMax == score) return 0;
		std::copy(cuts.begin(), cuts.end(), cuts_out);
		return cuts.size();
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		if (score_out) *score_out = vh::kCutPositionScoreMax;
		return 0;
	}
}

// find_cut_positions + find_matchings with the chunk walks of both on the GPU context `ctx`.  chunks: {cut search: walked on the
// GPU, left to the host; matching: walked, left}.  with_search = 0: the cut positions are given in cuts_out[0 .. n_cuts_in).
uint64_t v2mh_find_founders_gpu(void *h, void *ctx, uint64_t min_distance, uint32_t founder_count, int keep_ref_edges, unsigned threads,
	int with_search, uint64_t n_cuts_in, uint64_t *cuts_out, uint32_t *assigned_out, uint64_t assigned_capacity, uint32_t *score_out, uint64_t *chunks, char *err, size_t errlen)
{
	try {
		vh::gpu_context gpu(static_cast<v2m_ctx *>(ctx), vh::gpu_context::borrowed{});
		vh::gpu_founder_walker walker(gpu);
		auto const &g(HG(h).graph);
		std::vector<vh::u64> cuts;
		vh::u32 score(0);
		if (with_search) {
			score = vh::find_cut_positions(g, min_distance, cuts, threads, &walker);
			if (chunks) { chunks[0] = walker.chunks_walked; chunks[1] = walker.chunks_left; }
			if (score_out) *score_out = score;
			if (vh::kCutPositionScoreMax == score) return 0;
		} else {
			cuts.assign(cuts_out, cuts_out + n_cuts_in);
		}
		std::vector<vh::u32> assigned;
		walker.chunks_walked = walker.chunks_left = 0;
		if (!vh::find_matchings(g, cuts, founder_count, 0 != keep_ref_edges, assigned, threads, &walker)) return 0;
		if (chunks) { chunks[2] = walker.chunks_walked; chunks[3] = walker.chunks_left; }
		if (assigned.size() > assigned_capacity) return 0;
		std::copy(cuts.begin(), cuts.end(), cuts_out);
		std::copy(assigned.begin(), assigned.end(), assigned_out);
		return cuts.size();
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return 0;
	}
}

// The walked searches with the chunk walks done by the host's own edge-by-edge walker (founder.hh: make_host_founder_walker):
// the plumbing of find_cut_positions_walked / find_matchings_walked without a GPU.  chunks as in v2mh_find_founders_gpu.
uint64_t v2mh_find_founders_walked_on_host(void *h, uint64_t min_distance, uint32_t founder_count, int keep_ref_edges, unsigned threads, uint64_t max_copies,
	uint64_t *cuts_out, uint32_t *assigned_out, uint64_t assigned_capacity, uint32_t *score_out, uint64_t *chunks, char *err, size_t errlen)
{
	try {
		auto const &g(HG(h).graph);
		auto walker(vh::make_host_founder_walker(g, max_copies));
		std::vector<vh::u64> cuts;
		vh::u32 const score(vh::find_cut_positions(g, min_distance, cuts, threads, walker.get()));
		if (chunks) { chunks[0] = walker->chunks_walked; chunks[1] = walker->chunks_left; }
		if (score_out) *score_out = score;
		if (vh::kCutPositionScoreMax == score) return 0;
		std::vector<vh::u32> assigned;
		walker->chunks_walked = walker->chunks_left = 0;
		if (!vh::find_matchings(g, cuts, founder_count, 0 != keep_ref_edges, assigned, threads, walker.get())) return 0;
		if (chunks) { chunks[2] = walker->chunks_walked; chunks[3] = walker->chunks_left; }
		if (assigned.size() > assigned_capacity) return 0;
		std::copy(cuts.begin(), cuts.end(), cuts_out);
		std::copy(assigned.begin(), assigned.end(), assigned_out);
		return cuts.size();
	} catch (std::exception const &e) {      // nothing may cross the C boundary (an exception would end the caller's process)
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return 0;
	}
}

// find_matchings over the caller's cut positions with the host's own walker (what v2mh_find_founders_gpu does with with_search = 0, without a
// GPU).  Returns 1, or 0 with a message in err (a cut list find_matchings refuses) or without one (nothing to match).
int v2mh_find_matchings_walked_on_host(void *h, uint64_t const *cuts_in, uint64_t n_cuts, uint32_t founder_count, int keep_ref_edges, unsigned threads,
	uint32_t *assigned_out, uint64_t assigned_capacity, char *err, size_t errlen)
{
	try {
		auto const &g(HG(h).graph);
		auto walker(vh::make_host_founder_walker(g, UINT64_MAX));
		std::vector<vh::u64> const cuts(cuts_in, cuts_in + n_cuts);
		std::vector<vh::u32> assigned;
		if (!vh::find_matchings(g, cuts, founder_count, 0 != keep_ref_edges, assigned, threads, walker.get())) return 0;
		if (assigned.size() > assigned_capacity) return 0;
		std::copy(assigned.begin(), assigned.end(), assigned_out);
		return 1;
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return 0;
	}
}

uint64_t v2mh_find_founders(void *h, uint64_t min_distance, uint32_t founder_count, int keep_ref_edges,
	uint64_t *cuts_out, uint32_t *assigned_out, uint64_t assigned_capacity, uint32_t *score_out)
{
	return v2mh_find_founders_mt(h, min_distance, founder_count, keep_ref_edges, cuts_out, assigned_out, assigned_capacity, score_out, 1);
}

// The transpose's result (rows = edges, cols = copies, column-major words) for a graph whose builder ran without a GPU;
// the multi-threaded founder search reads copy prefixes from it.
void v2mh_set_paths_by_chrom_copy_and_edge(void *h, uint64_t const *words, uint64_t rows, uint64_t cols)
{
	auto &m(HG(h).graph.paths_by_chrom_copy_and_edge);
	m = vh::bit_matrix(rows, cols);
	std::copy(words, words + rows / 64 * cols, m.words.begin());
}

// Cut position files (founder.hh).  Return 0 on success, 1 with a message in err otherwise.
int v2mh_write_cut_positions(char const *path, uint64_t const *cuts, uint64_t n_cuts, uint64_t min_distance, uint32_t score, char *err, size_t errlen)
{
	try {
		vh::write_cut_positions({std::vector<vh::u64>(cuts, cuts + n_cuts), min_distance, score}, path);
		return 0;
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return 1;
	}
}

// cuts_out may be NULL to query the count (returned through *n_cuts); otherwise it must hold *n_cuts entries.
int v2mh_read_cut_positions(char const *path, uint64_t *cuts_out, uint64_t *n_cuts, uint64_t *min_distance, uint32_t *score, char *err, size_t errlen)
{
	try {
		auto const f(vh::read_cut_positions(path));
		if (cuts_out && *n_cuts >= f.cut_positions.size()) std::copy(f.cut_positions.begin(), f.cut_positions.end(), cuts_out);
		*n_cuts = f.cut_positions.size();
		if (min_distance) *min_distance = f.min_distance;
		if (score) *score = f.score;
		return 0;
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return 1;
	}
}


// shard_copies() of gpu_path.hh, for the test that it and vcf2multialign_amd/sharding.py agree on every boundary.
void v2mh_shard_copies(uint64_t n_copies, uint32_t world, uint32_t rank, uint64_t *first, uint64_t *end)
{
	auto const s(vh::shard_copies(n_copies, world, rank));
	*first = s.first;
	*end = s.end;
}

// chain_text() of output.hh (no GPU): the chain's bytes into dst when they fit `capacity`; returns their number, 0 for ops without any
// M (no chain), -1 with a message in err for ops that are none of M, I, D.
int64_t v2mh_chain_text(v2m_aln_op const *ops, uint64_t n_ops, char const *t_name, uint64_t t_size, char const *q_name, uint64_t q_size, uint64_t id,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		std::string const text(vh::chain_text(ops, n_ops, t_name, t_size, q_name, q_size, id));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// paf_text() of output.hh (no GPU), handed over as v2mh_chain_text hands over a chain: 0 for ops without any = / X (no line), -1 with a
// message in err for ops that are none of =, X, I, D.
int64_t v2mh_paf_text(v2m_aln_op const *ops, uint64_t n_ops, char const *t_name, uint64_t t_size, char const *q_name, uint64_t q_size,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		std::string const text(vh::paf_text(ops, n_ops, t_name, t_size, q_name, q_size));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// column_counts_text() of output.hh (no GPU), handed over as v2mh_chain_text hands over a chain; -1 with a message in err on failure.
int64_t v2mh_column_counts_text(uint64_t n_rows, v2m_column_count const *records, uint64_t n_records,
	uint64_t const *reference_positions, uint64_t const *aligned_positions, uint64_t node_count,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		std::string const text(vh::column_counts_text(n_rows, records, n_records, reference_positions, aligned_positions, node_count));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// distances_text() of output.hh (no GPU), handed over as v2mh_column_counts_text hands over its table; ids are n NUL-terminated
// strings; -1 with a message in err on failure.
int64_t v2mh_distances_text(char const *const *ids, uint64_t n_rows, uint32_t const *dist, uint64_t n_columns, uint64_t n_sites, int acgt_only,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		std::vector<std::string> names;
		for (uint64_t i(0); i < n_rows; ++i) names.emplace_back(ids[i]);
		std::string const text(vh::distances_text(names, dist, n_columns, n_sites, 0 != acgt_only));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// site_positions_text() of output.hh (no GPU), handed over as v2mh_column_counts_text hands over its table; -1 with a message in err
// on failure.
int64_t v2mh_site_positions_text(uint64_t const *columns, uint64_t n_sites, uint64_t const *reference_positions, uint64_t const *aligned_positions, uint64_t node_count,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		std::string const text(vh::site_positions_text(columns, n_sites, reference_positions, aligned_positions, node_count));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// site_ld_text() of output.hh (no GPU), handed over as v2mh_column_counts_text hands over its table; -1 with a message in err on failure.
int64_t v2mh_site_ld_text(uint64_t n_rows, uint64_t n_columns, v2m_ld_site const *sites, uint64_t n_sites, v2m_ld_pair const *pairs, uint64_t n_pairs,
	v2m_site_ld_params const *params, uint64_t const *reference_positions, uint64_t const *aligned_positions, uint64_t node_count,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!params) throw std::runtime_error("params is NULL");
		std::string const text(vh::site_ld_text(n_rows, n_columns, sites, n_sites, pairs, n_pairs, *params, reference_positions, aligned_positions, node_count));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// parse_decimal_fraction() of output.hh: 1 and the fraction in lowest terms, or 0
int v2mh_parse_decimal_fraction(char const *text, uint32_t *numerator, uint32_t *denominator)
{
	return text && numerator && denominator && vh::parse_decimal_fraction(text, *numerator, *denominator) ? 1 : 0;
}

// nj_tree_cpu() of output.hh (no GPU): the n - 2 records of the tree of dist (u32[n][pitch]) into nodes; 0, or -1 for a NULL pointer,
// n < 3, pitch < n or no memory.
int v2mh_nj_tree_cpu(uint32_t const *dist, uint64_t n, uint64_t pitch, v2m_nj_node *nodes)
{
	try {
		if (!dist || !nodes) return -1;
		vh::nj_tree_cpu(dist, n, pitch, nodes);
		return 0;
	} catch (std::exception const &) {
		return -1;
	}
}

// nj_newick_text() of output.hh (no GPU), handed over as v2mh_distances_text hands over its table; labels are n_leaves NUL-terminated
// strings; -1 with a message in err on failure.
int64_t v2mh_nj_newick_text(v2m_nj_node const *nodes, uint64_t n_leaves, char const *const *labels, char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!nodes || !labels) throw std::runtime_error("nodes or labels is NULL");
		std::vector<std::string> names;
		for (uint64_t i(0); i < n_leaves; ++i) names.emplace_back(labels[i]);
		std::string const text(vh::nj_newick_text(nodes, n_leaves, names));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// nj_newick_support_text() of output.hh (no GPU), handed over as v2mh_nj_newick_text hands over its text; support holds n_leaves - 3
// counts.
int64_t v2mh_nj_newick_support_text(v2m_nj_node const *nodes, uint64_t n_leaves, char const *const *labels, uint32_t const *support, char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!nodes || !labels) throw std::runtime_error("nodes or labels is NULL");
		std::vector<std::string> names;
		for (uint64_t i(0); i < n_leaves; ++i) names.emplace_back(labels[i]);
		std::string const text(vh::nj_newick_support_text(nodes, n_leaves, names, support));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// tree_parsimony_cpu() of output.hh (no GPU): the parsimony of the n_sites sites of bytes (u8[n][pitch]) on the tree of the n - 2 records;
// sites (n_sites), branch_changes (2 n - 3) and, when it fits capacity, mutations (may be NULL with capacity 0) are written.  The number
// of mutations, or -1 with a message in err for a NULL pointer or records that are no tree.
int64_t v2mh_tree_parsimony_cpu(unsigned char const *bytes, uint64_t n, uint64_t n_sites, uint64_t pitch, v2m_nj_node const *nodes, v2m_parsimony_site *sites,
	uint32_t *branch_changes, v2m_tree_mutation *mutations, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!nodes || !branch_changes || ((!bytes || !sites) && n_sites) || (!mutations && capacity)) throw std::invalid_argument("a pointer is NULL");
		return int64_t(vh::tree_parsimony_cpu(bytes, n, n_sites, pitch, nodes, sites, branch_changes, mutations, capacity));
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// nj_newick_parsimony_text() of output.hh (no GPU), handed over as v2mh_nj_newick_text hands over its text; branch_changes holds
// 2 n_leaves - 3 counts.
int64_t v2mh_nj_newick_parsimony_text(v2m_nj_node const *nodes, uint64_t n_leaves, char const *const *labels, uint32_t const *branch_changes, char *dst, uint64_t capacity,
	char *err, size_t errlen)
{
	try {
		if (!nodes || !labels) throw std::runtime_error("nodes or labels is NULL");
		std::vector<std::string> names;
		for (uint64_t i(0); i < n_leaves; ++i) names.emplace_back(labels[i]);
		std::string const text(vh::nj_newick_parsimony_text(nodes, n_leaves, names, branch_changes));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// tree_mutations_text() of output.hh (no GPU), handed over likewise; labels are n_leaves NUL-terminated strings.
int64_t v2mh_tree_mutations_text(v2m_tree_mutation const *mutations, uint64_t n_mutations, v2m_tree_site const *sites, uint64_t n_sites, char const *const *labels, uint64_t n_leaves,
	uint64_t const *reference_positions, uint64_t const *aligned_positions, uint64_t node_count, char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!labels) throw std::runtime_error("labels is NULL");
		std::vector<std::string> names;
		for (uint64_t i(0); i < n_leaves; ++i) names.emplace_back(labels[i]);
		std::string const text(vh::tree_mutations_text(mutations, n_mutations, sites, n_sites, names, reference_positions, aligned_positions, node_count));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// tree_sites_text() of output.hh (no GPU), handed over likewise.
int64_t v2mh_tree_sites_text(v2m_tree_site const *sites, uint64_t n_sites, uint64_t const *reference_positions, uint64_t const *aligned_positions, uint64_t node_count,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		std::string const text(vh::tree_sites_text(sites, n_sites, reference_positions, aligned_positions, node_count));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// window_diversity_cpu() of output.hh (no GPU).  0, or -1 with a message in err.
int v2mh_window_diversity_cpu(unsigned char const *rows_a, uint64_t n_a, unsigned char const *rows_b, uint64_t n_b, uint64_t L, uint64_t pitch, uint64_t const *bounds,
	uint64_t n_bins, void *bins, uint64_t *sfs, uint64_t *multiallelic, char *err, size_t errlen)
{
	try {
		if (!bounds || (!bins && n_bins) || (!rows_a && n_a && L) || (!rows_b && n_b)) throw std::invalid_argument("a pointer is NULL");
		vh::window_diversity_cpu(rows_a, n_a, rows_b, n_b, L, pitch, bounds, n_bins, bins, sfs, multiallelic);
		return 0;
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// diversity_values_of() of output.hh per record: out is double[n_windows][3] -- pi, theta_w, tajima_d; a quiet NaN where none exists.
int v2mh_window_diversity_values(v2m_diversity_bin const *windows, uint64_t n_windows, uint64_t n, double *out)
{
	if ((!windows || !out) && n_windows) return -1;
	for (uint64_t i(0); i < n_windows; ++i) {
		vh::diversity_values const v(vh::diversity_values_of(windows[i], n));
		out[3 * i] = v.pi; out[3 * i + 1] = v.theta_w; out[3 * i + 2] = v.tajima_d;
	}
	return 0;
}

// divergence_values_of() of output.hh per record: out is double[n_windows][2] -- dxy, fst.
int v2mh_window_divergence_values(v2m_diversity_between_bin const *between, v2m_diversity_bin const *windows_a, v2m_diversity_bin const *windows_b, uint64_t n_windows, double *out)
{
	if ((!between || !windows_a || !windows_b || !out) && n_windows) return -1;
	for (uint64_t i(0); i < n_windows; ++i) {
		vh::divergence_values const v(vh::divergence_values_of(between[i], windows_a[i], windows_b[i]));
		out[2 * i] = v.dxy; out[2 * i + 1] = v.fst;
	}
	return 0;
}

// window_diversity_text() of output.hh (no GPU), handed over as v2mh_nj_newick_text hands over its text.
int64_t v2mh_window_diversity_text(char const *group, uint64_t n, v2m_diversity_bin const *windows, uint64_t const *starts, uint64_t const *ends, uint64_t n_windows, int header,
	char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!group || ((!windows || !starts || !ends) && n_windows)) throw std::runtime_error("a pointer is NULL");
		std::string const text(vh::window_diversity_text(group, n, windows, starts, ends, n_windows, 0 != header));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// window_divergence_text() of output.hh (no GPU), handed over likewise.
int64_t v2mh_window_divergence_text(char const *group_a, char const *group_b, v2m_diversity_between_bin const *between, v2m_diversity_bin const *windows_a,
	v2m_diversity_bin const *windows_b, uint64_t const *starts, uint64_t const *ends, uint64_t n_windows, int header, char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!group_a || !group_b || ((!between || !windows_a || !windows_b || !starts || !ends) && n_windows)) throw std::runtime_error("a pointer is NULL");
		std::string const text(vh::window_divergence_text(group_a, group_b, between, windows_a, windows_b, starts, ends, n_windows, 0 != header));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// diversity_sfs_text() of output.hh (no GPU), handed over likewise; sfs holds n / 2 + 1 entries.
int64_t v2mh_diversity_sfs_text(char const *group, uint64_t n, uint64_t const *sfs, uint64_t multiallelic, int header, char *dst, uint64_t capacity, char *err, size_t errlen)
{
	try {
		if (!group || !sfs) throw std::runtime_error("a pointer is NULL");
		std::string const text(vh::diversity_sfs_text(group, n, sfs, multiallelic, 0 != header));
		if (dst && text.size() <= capacity) std::memcpy(dst, text.data(), text.size());
		return int64_t(text.size());
	} catch (std::exception const &e) {
		if (err && errlen) { std::strncpy(err, e.what(), errlen - 1); err[errlen - 1] = 0; }
		return -1;
	}
}

// nj_split_support() of csrc/nj_support.hpp (no GPU): support[t], t < n - 3, = the n_replicates trees of replicate_nodes (n - 2 records
// each) that hold the split of join record t of main_nodes.  0, or -1 for a NULL pointer, n < 3, records that are no tree, or no memory.
int v2mh_nj_split_support(uint64_t n, v2m_nj_node const *main_nodes, v2m_nj_node const *replicate_nodes, uint64_t n_replicates, uint32_t *support)
{
	try {
		if (!main_nodes || (!replicate_nodes && n_replicates) || (!support && n > 3)) return -1;
		vh::nj_split_support(n, main_nodes, replicate_nodes, n_replicates, support);
		return 0;
	} catch (std::exception const &) {
		return -1;
	}
}

} // extern "C"
