#include "gpu_path.hh"

#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <stdexcept>
#include <string>

#include <algorithm>

namespace v2m::host {

gpu_context::gpu_context(int device)
{
	int const rc(v2m_ctx_create(device, &m_ctx));
	if (V2M_OK != rc) throw gpu_error(rc, v2m_last_error(nullptr));
}

gpu_context::~gpu_context() { if (m_owned) v2m_ctx_destroy(m_ctx); }

void gpu_context::check(int rc) const
{
	if (V2M_OK != rc) throw gpu_error(rc, v2m_last_error(m_ctx));
}


input_file::input_file(char const *path) : m_path(path)
{
	unsigned char magic[2]{};
	{
		// only a regular file is probed: reading two bytes of a pipe (-r <(samtools faidx ...)) would take them from the path reader
		struct stat st;
		if (0 != ::stat(path, &st) || !S_ISREG(st.st_mode)) return;
		std::FILE *const f(std::fopen(path, "rb"));
		if (!f) return;                                                // the path readers report a missing file as before
		bool const got(2 == std::fread(magic, 1, 2, f));
		std::fclose(f);
		if (!got || 0x1f != magic[0] || 0x8b != magic[1]) return;      // plain text: no VCF or FASTA starts with these bytes
	}
	m_bgzf = true;
	m_file.reset(new mapped_file(path));
	int eof(0);
	if (V2M_OK != v2m_bgzf_scan(m_file->data, m_file->size, &m_members, &m_bytes, &eof))
		throw std::runtime_error(m_path + ": " + v2m_last_error(nullptr));
	m_eof = 0 != eof;
}

std::string_view input_file::inflate(gpu_context &gpu)
{
	if (!m_bgzf) throw std::logic_error(m_path + " is not BGZF");
	auto const t0(std::chrono::steady_clock::now());
	m_text.reset(new char[std::max<u64>(1, m_bytes)]);
	u64 n(0);
	int const rc(v2m_bgzf_decompress(gpu.get(), m_file->data, m_file->size, m_text.get(), m_bytes, &n));
	if (V2M_OK != rc) throw gpu_error(rc, m_path + ": " + v2m_last_error(gpu.get()));
	m_file.reset();                                                    // the compressed bytes are not needed any more
	m_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	return std::string_view(m_text.get(), n);
}


std::string_view input_file::compressed() const
{
	if (!m_bgzf || !m_file) throw std::logic_error(m_path + " is not BGZF, or has been inflated");
	return std::string_view(m_file->data, m_file->size);
}


void build_variant_graph_gpu_parsed(
	gpu_context &gpu, std::string const &name, std::string_view bytes, u64 text_bytes, sequence_type const &ref_seq, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, scan_statistics *scan_stats, u64 path_alignment)
{
	line_scanner const scanner([&](char const *chr, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user) {
		return v2m_vcf_scan(gpu.get(), bytes.data(), bytes.size(), chr, layout, chunk, user);
	});
	try {
		build_variant_graph_scanned(ref_seq, scanner, text_bytes, chr_id, graph, stats, delegate, scan_stats, path_alignment);
	} catch (scan_failed const &e) {
		throw gpu_error(e.code, name + ": " + v2m_last_error(gpu.get()));
	}
}


bit_matrix transpose_matrix(gpu_context &gpu, bit_matrix const &mat)
{
	if (0 == mat.cols) return bit_matrix{};                           // transpose_matrix.cc:48-49
	bit_matrix dst(mat.cols, mat.rows);
	gpu.check(v2m_transpose_bits(gpu.get(), mat.words.data(), mat.rows, mat.cols, dst.words.data()));
	return dst;
}


void transpose_paths(gpu_context &gpu, variant_graph &graph)
{
	graph.paths_by_chrom_copy_and_edge = transpose_matrix(gpu, graph.paths_by_edge_and_chrom_copy);
}


column_window columns_of_reference_range(variant_graph const &graph, u64 ref_len, u64 s, u64 e)
{
	auto const &rp(graph.reference_positions);
	auto const &ap(graph.aligned_positions);
	if (!(s < e && e <= ref_len) || rp.empty())
		throw std::invalid_argument("reference range [" + std::to_string(s) + ", " + std::to_string(e) + ") is empty or not within the reference (" + std::to_string(ref_len) + ")");
	auto const col([&](u64 p) -> u64 {
		if (p >= ref_len) return ap.back();
		u64 const n(u64(std::upper_bound(rp.begin(), rp.end(), p) - rp.begin()) - 1);   // rp[0] = 0 <= p
		return ap[n] + (p - rp[n]);
	});
	return {col(s), col(e)};
}


copy_shard shard_copies(u64 n_copies, u32 world, u32 rank)
{
	constexpr u64 granule(8);
	u64 const n_blocks((n_copies + granule - 1) / granule), base(n_blocks / world), extra(n_blocks % world);
	u64 const first_heavy(world - extra);
	u64 const b0(rank * base + (rank > first_heavy ? rank - first_heavy : 0));
	u64 const b1(b0 + base + (rank >= first_heavy ? 1 : 0));
	return {std::min(n_copies, granule * b0), std::min(n_copies, granule * b1)};
}


void upload_path_slice(gpu_context &gpu, variant_graph const &g, copy_shard shard)
{
	auto const &m(g.paths_by_edge_and_chrom_copy);
	gpu.check(v2m_upload_path_slice(gpu.get(), m.words.empty() ? nullptr : m.words.data(), m.rows, m.cols, shard.first, shard.end - shard.first));
}


void upload_path_blocks(gpu_context &gpu, variant_graph const &g, copy_interleave deal, u32 rank)
{
	auto const &m(g.paths_by_edge_and_chrom_copy);
	u64 const first(std::min<u64>(m.rows, deal.block * rank));
	gpu.check(v2m_upload_path_blocks(gpu.get(), m.words.empty() ? nullptr : m.words.data(), m.rows, m.cols, first, deal.block, deal.block * deal.world, m.rows));
}


void gpu_founder_walker::walk(u64 n_copies, u64 min_distance, std::vector<u32> const &cand_edge, std::vector<u64> const &cand_aligned,
	std::vector<u64> const &chunk_first, u32 const *start_order, u32 const *start_divergence,
	u64 capacity, u32 *trial_pred, u32 *trial_class, u64 *trial_end, u32 *status)
{
	m_gpu.check(v2m_pbwt_cut_trials(m_gpu.get(), n_copies, min_distance, cand_edge.size(), cand_edge.data(), cand_aligned.data(),
		chunk_first.size() - 1, chunk_first.data(), start_order, start_divergence, capacity, trial_pred, trial_class, trial_end, status));
}


void gpu_founder_walker::walk_streamed(u64 n_copies, u64 min_distance, std::vector<u32> const &cand_edge, std::vector<u64> const &cand_aligned,
	std::vector<u64> const &chunk_first, u32 const *start_order, u32 const *start_divergence,
	u64 capacity, u64 *trial_end, u32 *status, chunk_taker const &take)
{
	if (char const *const e = std::getenv("V2M_FOUNDER_ARRAYS")) if (*e && '0' != *e) {   // test knob: the array form of the call (v2m_pbwt_cut_trials), then the hand-over
		founder_walker::walk_streamed(n_copies, min_distance, cand_edge, cand_aligned, chunk_first, start_order, start_divergence, capacity, trial_end, status, take);
		return;
	}
	// the library calls back through C: what `take` throws is parked and thrown again once the call has returned
	struct relay { chunk_taker const &take; std::exception_ptr error; } state{take, nullptr};
	int const rc(v2m_pbwt_cut_trials_streamed(m_gpu.get(), n_copies, min_distance, cand_edge.size(), cand_edge.data(), cand_aligned.data(),
		chunk_first.size() - 1, chunk_first.data(), start_order, start_divergence, capacity, trial_end, status,
		[](void *user, uint64_t chunk, uint32_t chunk_status, uint32_t const *pred, uint32_t const *class_count, uint64_t n_pairs) -> int {
			relay &r(*static_cast<relay *>(user));
			try { r.take(std::size_t(chunk), chunk_status, pred, class_count, n_pairs); }
			catch (...) { r.error = std::current_exception(); return 1; }
			return 0;
		}, &state));
	if (state.error) std::rethrow_exception(state.error);
	m_gpu.check(rc);
}


void gpu_founder_walker::records(u64 n_copies, std::vector<u32> const &cut_edge, std::vector<u64> const &chunk_first_cut, std::vector<u32> const &start_edge,
	u32 const *start_order, u32 const *start_divergence, u64 pool_capacity, u32 *pool_lhs, u32 *pool_rhs, u32 *pool_size,
	u64 *rec_pool_end, u32 *rec_distinct, u32 *rec_first_class, u32 *rec_first_is_ref, u32 *status)
{
	m_gpu.check(v2m_pbwt_cut_records(m_gpu.get(), n_copies, cut_edge.size(), cut_edge.data(), chunk_first_cut.size() - 1, chunk_first_cut.data(), start_edge.data(),
		start_order, start_divergence, pool_capacity, pool_lhs, pool_rhs, pool_size, rec_pool_end, rec_distinct, rec_first_class, rec_first_is_ref, status));
}


void warm_up_sink(gpu_context &gpu, bool unaligned)
{
	// six REF rows into a sink that drops them: more than one slice of the sink path's default 512-MB slots whenever two
	// slices can occur at all, so both device slots and both pinned slots are allocated at the size later calls use
	u32 const copies[6] = {kPloidyMax, kPloidyMax, kPloidyMax, kPloidyMax, kPloidyMax, kPloidyMax};
	v2m_row_batch batch{};
	batch.n_rows = 6;
	batch.copy_index = copies;
	gpu.check(v2m_splice_rows(gpu.get(), &batch, unaligned ? V2M_SPLICE_UNALIGNED : 0u, [](void *, uint64_t, char const *, uint64_t) -> int { return 0; }, nullptr));
}


void upload_graph(gpu_context &gpu, sequence_type const &ref_seq, variant_graph const &g, bool with_paths)
{
	v2m_graph_view view{};
	view.node_count = g.node_count();
	view.edge_count = g.edge_count();
	view.reference_positions = g.reference_positions.data();
	view.aligned_positions = g.aligned_positions.data();
	view.alt_edge_targets = g.alt_edge_targets.data();
	view.alt_edge_count_csum = g.alt_edge_count_csum.data();
	view.alt_edge_label_offsets = g.alt_edge_label_offsets.data();
	view.alt_edge_label_bytes = g.alt_edge_label_bytes.data();
	auto const &paths(g.paths_by_chrom_copy_and_edge);
	view.paths_by_chrom_copy_and_edge = (!with_paths || paths.words.empty()) ? nullptr : paths.words.data();
	view.path_rows = with_paths ? paths.rows : 0;
	view.path_cols = with_paths ? paths.cols : 0;
	gpu.check(v2m_upload_graph(gpu.get(), &view, ref_seq.data(), ref_seq.size()));
}

} // namespace v2m::host
