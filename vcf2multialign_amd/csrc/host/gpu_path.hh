// gpu_path.hh -- the host's view of the GPU hot path: thin C++ wrappers over the C ABI (include/v2m_hip.h).
#pragma once

#include <memory>
#include <stdexcept>
#include <string>
#include <string_view>

#include "../../../include/v2m_hip.h"
#include "founder.hh"
#include "readers.hh"
#include "variant_graph.hh"

namespace v2m::host {

struct gpu_error : std::runtime_error {
	int code;
	gpu_error(int code_, std::string const &what) : std::runtime_error(what), code(code_) {}
};

class gpu_context {
public:
	explicit gpu_context(int device = 0);
	struct borrowed {};
	gpu_context(v2m_ctx *ctx, borrowed) : m_ctx(ctx), m_owned(false) {}   // somebody else's context (the Python binding's, in tests)
	~gpu_context();
	gpu_context(gpu_context const &) = delete;
	gpu_context &operator=(gpu_context const &) = delete;
	v2m_ctx *get() const { return m_ctx; }
	void check(int rc) const;   // throws gpu_error with v2m_last_error()
private:
	v2m_ctx *m_ctx{};
	bool m_owned{true};
};

// An input file of the driver (-a, -r), recognised by content: a regular file that starts with the gzip magic 1f 8b is BGZF, mapped and
// its framing checked at once (v2m_bgzf_scan, no device: std::runtime_error naming the file for gzip that is not BGZF and for broken
// framing); anything else, pipes included (nothing is read from them here), is plain text, left to the path readers (readers.hh)
// untouched.  inflate() decompresses a BGZF file on the
// GPU (v2m_bgzf_decompress) into host memory as large as the text; it replaces vcf::mmap_input (variant_graph.cc:133-134) and
// lb::read_single_fasta_sequence's file (vcf2multialign/main.cc:381) for compressed input.
class input_file {
public:
	explicit input_file(char const *path);
	bool bgzf() const { return m_bgzf; }
	u64 members() const { return m_members; }
	u64 bytes() const { return m_bytes; }
	bool ends_with_eof() const { return m_eof; }
	std::string_view inflate(gpu_context &gpu);   // BGZF only; throws gpu_error (a corrupt member: V2M_ERR_INVALID_ARGUMENT)
	std::string_view compressed() const;          // BGZF only, before inflate(): the mapped file, for a scan that inflates it slice by slice on the device (build_variant_graph_gpu_parsed)
	double inflate_seconds() const { return m_seconds; }
private:
	std::string m_path;
	bool m_bgzf{}, m_eof{};
	u64 m_members{}, m_bytes{};
	std::unique_ptr<mapped_file> m_file;
	std::unique_ptr<char[]> m_text;               // not value-initialised: its pages are first touched by the copy out of the pinned slots
	double m_seconds{};
};

// build_variant_graph with the genotype columns parsed on the GPU (readers.hh: build_variant_graph_scanned over v2m_vcf_scan): `bytes` is
// the whole VCF, BGZF or plain text, in host memory (a mapping); the text never reaches the host.  text_bytes: the decompressed size (a
// hint).  Throws what build_variant_graph throws, and gpu_error (`name`: the file, for the message) when the scan itself fails --
// V2M_ERR_UNSUPPORTED for a line longer than a slice or more than 32 768 chromosome copies: the caller then uses the text path.
void build_variant_graph_gpu_parsed(
	gpu_context &gpu, std::string const &name, std::string_view bytes, u64 text_bytes, sequence_type const &ref_seq, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, scan_statistics *scan_stats = nullptr, u64 path_alignment = 64);

// transpose_matrix (include/vcf2multialign/transpose_matrix.hh:14) on the GPU.
[[nodiscard]] bit_matrix transpose_matrix(gpu_context &gpu, bit_matrix const &mat);

// The last step of build_variant_graph (variant_graph.cc:453).
void transpose_paths(gpu_context &gpu, variant_graph &graph);

// Makes `graph` + `ref_seq` the resident graph of the context.  with_paths = false leaves the path matrix out (it then
// comes from upload_path_slice()).
void upload_graph(gpu_context &gpu, sequence_type const &ref_seq, variant_graph const &graph, bool with_paths = true);

// The column window of the 0-based half-open reference range [s, e) (0 <= s < e <= ref_len): [col(s), col(e)) with
// col(p) = aligned_positions[n] + (p - reference_positions[n]) for the last node n with reference_positions[n] <= p and
// col(ref_len) = the aligned length -- what v2m_set_column_window() takes.  Throws std::invalid_argument for a range outside that.
struct column_window { u64 begin{}, end{}; };
column_window columns_of_reference_range(variant_graph const &graph, u64 ref_len, u64 s, u64 e);

// Pays the sink path's one-off costs ahead of time (a gigabyte of pinned host memory: 0.15 s of hipHostMalloc, the device
// slots, the templates) by splicing a few REF rows into a sink that drops them.  For callers that have something else
// to do before the first real row (the founder search); needs an uploaded graph.
void warm_up_sink(gpu_context &gpu, bool unaligned);

// The chromosome copies [first, end) a GPU owns when `n_copies` copies are sharded over `world` GPUs (SURVEY.md section 8e;
// the same rule as vcf2multialign_amd/sharding.py:shard_copies): contiguous blocks of whole bytes of the bit-packed path
// matrix (8 copies), the blocks that do not divide evenly go to the last GPUs because the first one also carries the REF row.
struct copy_shard { u64 first{}, end{}; };
copy_shard shard_copies(u64 n_copies, u32 world, u32 rank);

// This GPU's copies [first, end) of graph.paths_by_edge_and_chrom_copy: uploaded (only those bytes), transposed on the
// GPU and bound as the resident graph's path matrix (v2m_upload_path_slice).  Row batches for this context then use copy
// indices relative to `first`.  Nothing comes back to the host.
void upload_path_slice(gpu_context &gpu, variant_graph const &graph, copy_shard shard);

// Chromosome copies dealt to `world` GPUs in blocks of `block` copies, round-robin (v2m_upload_path_blocks): GPU `rank` owns the
// copies c with (c / block) % world == rank.  This is the sharding for outputs that have to leave in row order -- pipes,
// unaligned A2M, one file per sequence with a delegate that counts them -- where contiguous shards would leave all GPUs but
// one waiting for their turn: with blocks dealt round-robin every GPU always has rows that are due soon.
struct copy_interleave {
	u64 block{8};     // copies per block: a multiple of 8 (whole bytes of the bit-packed columns)
	u32 world{1};
	u32 owner(u64 copy) const { return u32((copy / block) % world); }
	u64 local(u64 copy) const { return (copy / (block * world)) * block + copy % block; }   // the copy's index in its owner's matrix
};
void upload_path_blocks(gpu_context &gpu, variant_graph const &graph, copy_interleave deal, u32 rank);

// The chunk walks of the founder searches on the GPU (v2m_pbwt_cut_trials, v2m_pbwt_cut_records).  The context must hold the
// uploaded graph with its path matrix (upload_graph(..., true)).
class gpu_founder_walker final : public founder_walker {
public:
	explicit gpu_founder_walker(gpu_context &gpu) : m_gpu(gpu) {}
	u64 max_copies() const override { return 20480; }          // v2m_pbwt_cut_trials: csrc/founder_kernels.hpp kPbwtMaxCopies
	u64 max_copies_records() const override { return 20480; }  // v2m_pbwt_cut_records: kPbwtMaxCopiesRecords (its class arrays in LDS up to 12 288 copies, in device memory above)
	std::size_t preferred_chunks() const override { return 256; }   // one workgroup per chunk, 1024 threads each: one round over 256 CUs
	void walk(u64 n_copies, u64 min_distance, std::vector<u32> const &cand_edge, std::vector<u64> const &cand_aligned,
		std::vector<u64> const &chunk_first, u32 const *start_order, u32 const *start_divergence,
		u64 capacity, u32 *trial_pred, u32 *trial_class, u64 *trial_end, u32 *status) override;
	void walk_streamed(u64 n_copies, u64 min_distance, std::vector<u32> const &cand_edge, std::vector<u64> const &cand_aligned,
		std::vector<u64> const &chunk_first, u32 const *start_order, u32 const *start_divergence,
		u64 capacity, u64 *trial_end, u32 *status, chunk_taker const &take) override;   // v2m_pbwt_cut_trials_streamed
	void records(u64 n_copies, std::vector<u32> const &cut_edge, std::vector<u64> const &chunk_first_cut, std::vector<u32> const &start_edge,
		u32 const *start_order, u32 const *start_divergence, u64 pool_capacity, u32 *pool_lhs, u32 *pool_rhs, u32 *pool_size,
		u64 *rec_pool_end, u32 *rec_distinct, u32 *rec_first_class, u32 *rec_first_is_ref, u32 *status) override;
private:
	gpu_context &m_gpu;
};
typedef gpu_founder_walker gpu_cut_trial_walker;

} // namespace v2m::host
