// v2m_hip.hip -- implementation of the C ABI in include/v2m_hip.h for MI355X (gfx950).
//
// Host side of the device path: validates and narrows the variant graph, derives the device
// tables, owns all HBM allocations and the two HIP streams (compute + D2H), and launches the
// kernels in kernels.hpp.  There is no CPU fallback anywhere in this file: every entry point
// either runs on the GPU or returns an error.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include <type_traits>
#include <unordered_map>

#include "../../include/v2m_hip.h"
#include "kernels.hpp"
#include "founder_kernels.hpp"
#include "bgzf_kernels.hpp"
#include "vcf_kernels.hpp"
#include "distance_kernels.hpp"
#include "bootstrap_kernels.hpp"
#include "parsimony_kernels.hpp"
#include "diversity_kernels.hpp"
#include "site_kernels.hpp"
#include "ld_kernels.hpp"
#include "nj_kernels.hpp"
#include "nj_support.hpp"

using v2m::u32;
using v2m::u64;

namespace {

thread_local std::string g_create_error;

#ifdef V2M_CHECKED_BUILD
// Checked build (kernels.hpp): device memory and pinned staging are filled with a pattern derived from V2M_POISON_SEED before use, so
// that a kernel or a copy that reads what nobody wrote in this call sees garbage instead of the previous call's (usually right) bytes.
std::atomic<u32> g_poison_seed{0x9E3779B9u};
std::atomic<u32> g_poison_salt{1};

u32 poison_mix(u32 h)
{
	h ^= h >> 16; h *= 0x7FEB352Du;
	h ^= h >> 15; h *= 0x846CA68Bu;
	return h ^ (h >> 16);
}

// After a device-wide synchronize (nothing in flight is overwritten), and synchronized again.
hipError_t poison_device(void *p, size_t n)
{
	if (!p || !n) return hipSuccess;
	hipError_t st(hipDeviceSynchronize());
	if (hipSuccess != st) return st;
	u64 const words(n / 4);
	unsigned const blocks(unsigned(std::min<u64>(4096, words / 256 + 1)));
	hipLaunchKernelGGL(v2m::poison_fill_kernel, dim3(blocks), dim3(256), 0, 0, static_cast<unsigned char *>(p), u64(n), g_poison_seed.load(), poison_mix(g_poison_salt++));
	if (hipSuccess != (st = hipGetLastError())) return st;
	return hipDeviceSynchronize();
}

void poison_host(void *p, size_t n)
{
	if (!p) return;
	u32 const salt(poison_mix(g_poison_salt++ ^ g_poison_seed.load()));
	unsigned char *const b(static_cast<unsigned char *>(p));
	for (size_t i(0); i < n / 4; ++i) { u32 const w(poison_mix(salt ^ u32(i) * 0x9E3779B1u)); std::memcpy(b + 4 * i, &w, 4); }
	for (size_t i(n / 4 * 4); i < n; ++i) b[i] = (unsigned char) poison_mix(salt + u32(i));
}
#define V2M_POISON_HOST(p, n) poison_host((p), (n))
#else
#define V2M_POISON_HOST(p, n) ((void) 0)
#endif

struct dev_buf {
	void *p{};
	size_t bytes{};
	dev_buf() = default;
	dev_buf(dev_buf const &) = delete;
	dev_buf &operator=(dev_buf const &) = delete;
	~dev_buf() { reset(); }
	void reset() { if (p) (void) hipFree(p); p = nullptr; bytes = 0; }
	hipError_t ensure(size_t n)
	{
		if (n <= bytes) return hipSuccess;
		reset();
		if (0 == n) return hipSuccess;
		hipError_t const st(hipMalloc(&p, n));
		if (hipSuccess == st) bytes = n; else p = nullptr;
#ifdef V2M_CHECKED_BUILD
		if (hipSuccess == st) return poison_device(p, n);
#endif
		return st;
	}
	template <typename T> T *as() const { return static_cast<T *>(p); }
};

// Per-call scratch: in the checked build every ensure() -- each call or slice takes its scratch that way -- fills the buffer again.
struct scratch_buf : dev_buf {
	hipError_t ensure(size_t n)
	{
		bool const fresh(n > bytes);
		hipError_t const st(dev_buf::ensure(n));
#ifdef V2M_CHECKED_BUILD
		if (hipSuccess == st && !fresh) return poison_device(p, bytes);
#else
		(void) fresh;
#endif
		return st;
	}
};

struct pinned_buf {
	void *p{};
	size_t bytes{};
	~pinned_buf() { reset(); }
	void reset() { if (p) (void) hipHostFree(p); p = nullptr; bytes = 0; }
	hipError_t ensure(size_t n)
	{
		if (n <= bytes) return hipSuccess;
		reset();
		if (0 == n) return hipSuccess;
		hipError_t const st(hipHostMalloc(&p, n, hipHostMallocDefault));
		if (hipSuccess == st) bytes = n; else p = nullptr;
		return st;
	}
	template <typename T> T *as() const { return static_cast<T *>(p); }
};

struct event_pair { hipEvent_t begin{}, end{}; };

} // namespace


// One pinned slot of the context's ring: the rows of one slice, and how many of them a v2m_splice_rows_held sink still holds.  A
// row's hold IS its slot (include/v2m_hip.h: v2m_row_hold), so that a release is one decrement under the ring's mutex from whatever
// thread.
struct held_ring_state {
	std::mutex mutex;
	std::condition_variable released;
};

struct v2m_row_hold {
	pinned_buf host;
	hipEvent_t copied{};                // the slice's D2H copy has landed in `host`
	uint64_t outstanding{};             // delivered rows not yet released (under ring->mutex)
	held_ring_state *ring{};
};


// The edge words a row call resolves, [lo, hi), and the scratch layout: a row holds words [restart, restart + stride) (the look-back
// of the words' restart points stays within them), so word w of row r is at d_eff + r * stride + (w - restart).
struct word_range { u64 restart, lo, hi, stride; };

// The columns [begin, end) every row call produces, with what the splice kernels take for them: the REF row with '-' as padding and
// the one with 0 (unaligned mode, built on first use), the tables of the view's tiles (tile t = columns begin + t * kTileBytes on),
// and the edge words resolve decides.
struct row_view {
	u64 begin{}, end{};
	u64 max_unaligned{};                // the longest unaligned body a row of the view can have
	u32 n_tiles{};
	dev_buf d_template, d_template0;
	bool has_template0{};
	dev_buf d_edge_begin, d_cross_offsets, d_cross_edges;
	word_range words{};
	u64 length() const { return end - begin; }
};


struct v2m_ctx {
	int device{};
	u32 n_cus{256};          // compute units of the device (the lines16 transpose sizes its spans by it)
	hipStream_t stream{};
	hipStream_t copy_stream{};
	std::string err;

	// profiling
	bool profiling{};
	std::vector<event_pair> events[V2M_KERNEL_LIMIT];
	std::vector<event_pair> free_events;

	// graph
	bool has_graph{};
	u64 n_nodes{}, n_edges{}, ref_len{}, aligned_len{}, label_bytes{};
	bool has_nul_byte{};                // ref_seq or a label holds a 0 byte: the unaligned kernels' padding marker (kernels.hpp), so --unaligned refuses
	std::vector<u32> h_csum;            // alt_edge_count_csum narrowed, [N + 1]
	std::vector<u32> h_tgt_prefix_max;  // [E + 1]: max target over edges < e (cut validation)
	dev_buf d_ref, d_ref_pos, d_aln_pos, d_spans, d_patches, d_labels, d_overlappable;
	dev_buf d_ovl_rank, d_blocker_masks;   // per word: overlappable edges before it; per overlappable edge: who can block it
	// host copies of what v2m_set_column_window derives a window's tables from
	std::vector<u32> h_aln_pos, h_tile_edge_begin, h_cross_offsets, h_cross_edges;
	std::vector<v2m::edge_patch> h_patches;
	std::vector<u64> h_overlappable;

	// whole rows (v2m_upload_graph) and the column window of v2m_set_column_window; row calls produce the columns of the view in force,
	// and the window's is in force only while `windowed`, which also picks the window instances of the splice kernels
	row_view whole, window;
	bool windowed{};
	row_view &view() { return set_call ? set.view : windowed ? window : whole; }
	row_view const &view() const { return set_call ? set.view : windowed ? window : whole; }

	// The window set (v2m_set_window_set): a third view, in force only inside the set calls (`set_call`), which the row calls never see.
	// Its "columns" are a record's bytes up to the end of the last slot; its tiles are numbered across the windows in set order and carry
	// their columns, edge range end and record offset in tables of their own (kernels.hpp: set_tile_tables); the scan of the unaligned
	// tile counts is segmented by tile_window / first_tile / slot_offset32.
	struct window_set {
		row_view view;
		u64 n_windows{}, pitch{}, mean_tile_bytes{};
		std::vector<u32> lengths;           // [n_windows] the windows' lengths: every row's lengths in aligned mode
		dev_buf d_col_begin, d_col_end, d_record_offset, d_edge_end, d_tile_window, d_first_tile, d_slot_offset32;
	} set;
	bool has_set{}, set_call{};
	scratch_buf d_set_tile_offsets, d_set_lengths[2];   // unaligned: the tiles' destinations; [rows][n_windows] lengths of a slice, two in turn (s & 1)
	int set_lengths_slot{};
	// distinct pieces (v2m_splice_window_set_distinct): a slice's keys, the windows' item table and lengths, a round's gather or verify
	// items and its flags, with their pinned staging (keys and lengths down, items up, flags down); the pool belongs to the call
	scratch_buf d_distinct_keys, d_distinct_windows, d_distinct_items, d_distinct_flags;
	pinned_buf h_distinct_keys, h_distinct_items, h_distinct_flags;

	// paths_by_chrom_copy_and_edge
	u64 const *d_paths{};
	dev_buf owned_paths;
	dev_buf d_slice_src;     // v2m_upload_path_slice: the un-transposed slice (released after the transpose)
	u64 path_rows{}, path_cols{};
	u64 path_pitch{};        // words from one copy's column to the next (path_rows / 64 for caller-supplied matrices)
	// founder search: the bound matrix transposed back to edge-major bits (paths_by_edge_and_chrom_copy), made by the first of the
	// v2m_pbwt_* calls after a matrix is bound and kept for the following ones (one founder run makes two); dropped with the binding
	dev_buf d_by_edge;
	bool by_edge_valid{};

	struct transpose_pick { u64 rows, cols, src_pitch, dst_pitch; std::string kernel; };
	std::vector<transpose_pick> transpose_choice;   // per matrix shape: which transpose kernel measured fastest

	// store flavour of the aligned splice: -1 = not calibrated yet, 0 = plain, 1 = nontemporal
	int store_mode{-1};
	int unaligned_store_mode{-1};   // the same for the unaligned splice
	std::string info;

	// per-call scratch
	// segment tables of the row batch being resolved: two pinned staging areas used in turn, so that the host can prepare and
	// queue the next slice while the previous one is still running (each area is reused only after its uploads have left it)
	pinned_buf h_row_stage[2];
	hipEvent_t ev_row_stage[2]{};
	bool row_stage_in_flight[2]{};
	int row_stage_next{};
	scratch_buf d_resolve_queue, d_resolve_count;   // (row, word) pairs the streaming resolve pass leaves to the dense one
	scratch_buf d_eff, d_row_bits, d_seg_offsets, d_seg_edge_begin, d_seg_copy, d_sums, d_lengths, d_needs_serial, d_tile_counts, d_row_lengths;
	scratch_buf ring[2];
	// row alignment ops (v2m_row_ops): the reference bytes before each tile of the whole view (once per upload), a slice's per-tile
	// breakpoint words / carried classes, op offsets, per-row op counts and bases, its breakpoint records, and their pinned staging
	dev_buf d_ops_ref_before;
	bool has_ops_ref_before{};
	scratch_buf d_ops_info, d_ops_offsets, d_ops_counts, d_ops_base, d_ops_out;
	pinned_buf h_ops_stage, h_ops_out;
	std::vector<v2m_aln_op> ops_row;
	// column counts (v2m_column_counts): the sink form's table, the staged byte lanes of a call whose slices hold few rows, a column
	// range's block counts and total, its records (two, used in turn) and the total's pinned staging (two likewise).  The table, the
	// block counts, the total and its staging are also what select_sites_count takes for every analysis that selects sites (pair
	// distances, variable sites, site LD, parsimony); the staging's second word is the weighted pair distances' OR of the weights
	scratch_buf d_column_table, d_column_stage, d_column_blocks, d_column_total, d_column_records[2];
	pinned_buf h_column_total;
	// pair distances (v2m_pair_distances): the site list (select_rule_sites_emit), a pass's bit planes, and the host form's matrix
	scratch_buf d_dist_sites, d_dist_planes, d_dist_matrix;
	// bootstrap (v2m_pair_distances_weighted, v2m_bootstrap_distances, v2m_nj_bootstrap): explicit weights by column, a replicate's
	// weights by site rank, their 32 bit slices, the OR of the weights, and a replicate's matrix
	scratch_buf d_boot_column_weights, d_boot_weights, d_boot_slices, d_boot_any, d_boot_matrix;
	// neighbour joining (v2m_nj_tree[_of_distances]): the working matrix, R, the ids, the row minima and the records
	scratch_buf d_nj_matrix, d_nj_sums, d_nj_ids, d_nj_best, d_nj_nodes;
	// parsimony (v2m_parsimony_of_sites, v2m_tree_parsimony): the sets, the join table, the workgroups' steps and the call's total with
	// its pinned staging, and for the host form a range's leaf bytes, the branch counters and a range's records and mutations (two, in turn)
	scratch_buf d_fitch_sets, d_fitch_joins, d_fitch_blocks, d_fitch_total, d_fitch_bytes, d_fitch_branches, d_fitch_sites[2], d_fitch_mutations[2];
	pinned_buf h_fitch_total;
	// window diversity (v2m_diversity_of_counts, v2m_window_diversity): the bounds, relative to the table; the count of multiallelic
	// columns with its pinned staging; and for the host form the second group's table, the records and the spectrum
	scratch_buf d_diversity_bounds, d_diversity_multiallelic, d_diversity_table_b, d_diversity_records, d_diversity_sfs;
	pinned_buf h_diversity_multiallelic;
	// variable sites (v2m_variable_sites) and parsimony: the site list (select_rule_sites_emit), the host form's gathered slices (two,
	// used in turn), the list's pinned staging (fetch_site_columns)
	scratch_buf d_site_columns, d_site_bytes[2];
	pinned_buf h_site_columns;
	// site LD (v2m_site_ld): the site list and the records, the bit planes, the (site, tile) cells, the strips' totals and bases, the
	// host form's pairs of a range (two, used in turn), and the pinned staging of the records and of the totals and bases
	scratch_buf d_ld_sites, d_ld_records, d_ld_planes, d_ld_cells, d_ld_totals, d_ld_bases, d_ld_pairs[2];
	pinned_buf h_ld_records, h_ld_strips;
	// pinned slots: the rows of v2m_splice_rows[_held] (a slot is kept until the sink has released its rows); slots 0 and 1 also stage
	// the BGZF members and v2m_upload_path_blocks' columns
	held_ring_state held_state;
	std::vector<std::unique_ptr<v2m_row_hold>> host_slots;
	pinned_buf trials_stage[2];   // v2m_pbwt_cut_trials_streamed: the pairs' way back to the host
	// BGZF (V2M_SPLICE_BGZF, v2m_bgzf_compress): one 64-KiB member slot per block of a slice, the members' sizes and scanned offsets,
	// the dense members of a slice (two: one crossing the link while the next is compacted) and their row extents on the host
	scratch_buf d_bgzf_slots, d_bgzf_sizes, d_bgzf_offsets, d_bgzf_table, d_bgzf_dense[2], d_bgzf_in;
	pinned_buf h_bgzf_table[2];
	hipEvent_t ev_compute[2]{};
	// BGZF input (v2m_bgzf_decompress): a slice's members and their member / output offsets, its output and the members' statuses, two
	// of each (slice s + 1 crosses the link while slice s is inflated)
	scratch_buf d_inflate_in[2], d_inflate_out[2], d_inflate_status[2];
	hipEvent_t ev_inflate_in[2]{};
	// VCF scan (v2m_vcf_scan): the text of a slice, two buffers used in turn (the line a slice ends in is carried into the other one's
	// front), the slice's compressed members, and what the passes of vcf_kernels.hpp leave
	dev_buf d_vcf_text[2];
	scratch_buf d_vcf_in, d_vcf_status, d_vcf_tiles, d_vcf_tile_offsets, d_vcf_line_start, d_vcf_lines, d_vcf_gt_off, d_vcf_flags, d_vcf_tmp_begin,
		d_vcf_tmp_columns, d_vcf_totals, d_vcf_heads, d_vcf_columns, d_vcf_layout, d_vcf_wanted;
};


namespace {

int fail(v2m_ctx *ctx, int code, char const *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	std::vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	if (ctx) ctx->err = buf; else g_create_error = buf;
	return code;
}

#define V2M_HIP_TRY(ctx, expr)                                                              \
	do {                                                                                    \
		hipError_t const st_ = (expr);                                                      \
		if (hipSuccess != st_) {                                                            \
			int const code_ = (hipErrorOutOfMemory == st_) ? V2M_ERR_OUT_OF_MEMORY : V2M_ERR_HIP; \
			return fail(ctx, code_, "%s failed: %s", #expr, hipGetErrorString(st_));       \
		}                                                                                   \
	} while (0)


// Brackets a launch with events when profiling is on.
struct timed_launch {
	v2m_ctx *ctx;
	int kernel;
	event_pair ev{};
	bool active{};

	timed_launch(v2m_ctx *c, int k) : ctx(c), kernel(k)
	{
		if (!ctx->profiling) return;
		if (!ctx->free_events.empty()) { ev = ctx->free_events.back(); ctx->free_events.pop_back(); }
		else if (hipSuccess != hipEventCreate(&ev.begin) || hipSuccess != hipEventCreate(&ev.end)) return;
		active = (hipSuccess == hipEventRecord(ev.begin, ctx->stream));
	}
	~timed_launch()
	{
		if (!active) return;
		(void) hipEventRecord(ev.end, ctx->stream);
		ctx->events[kernel].push_back(ev);
	}
};


template <typename T>
int upload_vec(v2m_ctx *ctx, dev_buf &dst, std::vector<T> const &src, size_t min_bytes = 16)
{
	size_t const bytes(std::max(src.size() * sizeof(T), min_bytes));
	V2M_HIP_TRY(ctx, dst.ensure(bytes));
	if (!src.empty())
		V2M_HIP_TRY(ctx, hipMemcpyAsync(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
	return V2M_OK;
}


// Events that destroy themselves, and a guard that puts ctx->profiling back: the calibration paths below return early
// on any HIP error.
struct scoped_events {
	std::vector<hipEvent_t> ev;
	~scoped_events() { for (auto e : ev) (void) hipEventDestroy(e); }
	hipError_t create(std::size_t n)
	{
		for (std::size_t i(0); i < n; ++i) {
			hipEvent_t e{};
			hipError_t const st(hipEventCreate(&e));
			if (hipSuccess != st) return st;
			ev.push_back(e);
		}
		return hipSuccess;
	}
	hipEvent_t operator[](std::size_t i) const { return ev[i]; }
};

struct scoped_profiling_off {
	v2m_ctx *ctx;
	bool was;
	explicit scoped_profiling_off(v2m_ctx *c) : ctx(c), was(c->profiling) { c->profiling = false; }
	~scoped_profiling_off() { ctx->profiling = was; }
};


// 1-D grids in XCD chunks (kernels.hpp: xcd_chunked_item); xcd = false keeps the plain dispatch order (tuning A/B).
struct xcd_grid { unsigned blocks; u32 items_per_xcd; };

bool make_xcd_grid(u64 n_items, bool xcd, xcd_grid &g)
{
	u64 const per((n_items + 7) / 8), blocks(xcd ? per * 8 : n_items);
	if (0 == n_items || blocks > 0x7FFFFFFFull) return false;
	g.blocks = unsigned(blocks);
	g.items_per_xcd = xcd ? u32(per) : 0u;
	return true;
}

// Which dimension of the panel grid runs fastest in item order: 0 = the shorter one (both kinds of neighbours stay close
// in time), 1 = row panels, 2 = column panels / spans.
u32 rows_fastest_for(int order, u64 n_row_panels, u64 n_col_panels)
{
	if (1 == order) return 1;
	if (2 == order) return 0;
	return n_row_panels <= n_col_panels ? 1u : 0u;
}

template <int kR, int kC>
int launch_transpose_shape(v2m_ctx *ctx, u64 const *d_src, u64 SW, u64 DW, u64 SP, u64 DP, u64 *d_dst, bool xcd, int order)
{
	u64 const P((SW + kR - 1) / kR), Q((DW + kC - 1) / kC);
	xcd_grid g;
	if (P > 0xFFFFFFFFull || Q > 0xFFFFFFFFull || !make_xcd_grid(P * Q, xcd, g))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "matrix too large for one transpose launch (%llu x %llu bits)", (unsigned long long) (SW * 64), (unsigned long long) (DW * 64));
	{
		timed_launch tl(ctx, V2M_KERNEL_TRANSPOSE);
		hipLaunchKernelGGL((v2m::transpose_bits_kernel<kR, kC>), dim3(g.blocks), dim3(v2m::kTrThreads), 0, ctx->stream, d_src, d_dst, SW, DW, SP, DP, u32(P), u32(Q), g.items_per_xcd, rows_fastest_for(order, P, Q));
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}

template <int kDepth, int kSlabCols, int kWaves = 4, int kTsR = 16, int kTsC = 16, bool kLean = true>
int launch_transpose_stream(v2m_ctx *ctx, u64 const *d_src, u64 SW, u64 DW, u64 SP, u64 DP, u64 *d_dst, bool xcd, int order)
{
	u64 const P((SW + kTsR - 1) / kTsR), Q((DW + kTsC - 1) / kTsC);
	xcd_grid g;
	if (P > 0xFFFFFFFFull || Q > 0xFFFFFFFFull || !make_xcd_grid(P * Q, xcd, g)) return fail(ctx, V2M_ERR_UNSUPPORTED, "matrix too large for one transpose launch");
	{
		timed_launch tl(ctx, V2M_KERNEL_TRANSPOSE);
		hipLaunchKernelGGL((v2m::transpose_bits_stream_kernel<kDepth, kSlabCols, kWaves, kTsR, kTsC, kLean>), dim3(g.blocks), dim3(64 * kWaves), 0, ctx->stream, d_src, d_dst, SW, DW, SP, DP, u32(P), u32(Q), g.items_per_xcd, rows_fastest_for(order, P, Q));
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}

// The sector-aligned streaming kernel: kR row-words per workgroup on kW waves, kS-word sectors, kD steps of prefetch,
// spans of `span_groups` column groups (0 = default).
template <int kR, int kW, int kS, int kD, bool kFast, bool kNT>
int launch_transpose_ring(v2m_ctx *ctx, u64 const *d_src, u64 SW, u64 DW, u64 SP, u64 DP, u64 *d_dst, u64 span_groups, bool xcd, int order)
{
	if (0 == span_groups) span_groups = 64;
	span_groups = (span_groups + kS - 1) / kS * kS;
	u64 const P((SW + kR - 1) / kR), NS((DW + span_groups - 1) / span_groups);
	xcd_grid g;
	if (P > 0xFFFFFFFFull || NS > 0xFFFFFFFFull || span_groups > 0x7FFFFFFFull || DW > 0xFFFFFFFFull || !make_xcd_grid(P * NS, xcd, g))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "matrix too large for one transpose launch");
	{
		timed_launch tl(ctx, V2M_KERNEL_TRANSPOSE);
		hipLaunchKernelGGL((v2m::transpose_bits_ring_kernel<kR, kW, kS, kD, kFast, kNT>), dim3(g.blocks), dim3(64 * kW), 0, ctx->stream,
			d_src, d_dst, SW, DW, SP, DP, u32(P), u32(NS), u32(span_groups), g.items_per_xcd, rows_fastest_for(order, P, NS));
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}

// The whole-line streaming kernel: kTsR row-words per workgroup on kWaves waves, spans of `span_blocks` blocks of 16 column groups.
// span_blocks = 0: chosen here.  Long spans leave fewer lines written in two pieces, short ones more workgroups to balance: a
// whole destination column per workgroup where columns are short and there are plenty of panels (the inverse direction of a
// path matrix: 5 blocks at config 3, 20 at config 5), otherwise the longest of 32 / 16 / 8 / 4 blocks that still leaves
// 1024 workgroups = two rounds over the chip (measured, config 3 forward with its 10 panels: 8 or 10 blocks 0.295-0.306 ms,
// 4-7 blocks 0.300-0.322, 12 and more 0.334-0.347; config 5 forward: 16-32).
template <int kWaves, int kDepth, int kTsR = 8, int kSlabRows = 32, bool kMayMerge = false>
int launch_transpose_lines(v2m_ctx *ctx, u64 const *d_src, u64 SW, u64 DW, u64 SP, u64 DP, u64 *d_dst, u64 span_blocks, bool xcd, int order)
{
	u64 const P((SW + kTsR - 1) / kTsR), NB((DW + 15) / 16);
	if (0 == span_blocks && 16 == kTsR) {
		// lines16 (two tiles per wave: 185-253 VGPRs, ONE workgroup per CU): the grid is cut for whole rounds over the chip.  Among the span
		// counts that leave at least 4 blocks per span, the one with the best (share of the CUs busy in the last round) x (share of the lines a
		// span writes whole: K / (K + 1)); fewer, longer spans on a tie.  Config 3 forward (5 panels x 977 blocks): 49 spans of 20 blocks =
		// 245 workgroups, one round (measured: 20 blocks 0.263-0.286 ms, 10 blocks 0.276-0.302, 8 / 13 / 16 blocks -- 2.4, 1.5, 1.2 rounds --
		// 0.32-0.38); config 5 forward (20 panels x 6093 blocks): 51 spans of 120; whole columns when there are more panels than CUs.
		u64 const n_cus(std::max<u32>(1, ctx->n_cus));
		u64 const max_spans(std::max<u64>(1, std::min<u64>(NB / 4, 4 * n_cus / std::max<u64>(1, P) + 1)));
		double best(-1);
		for (u64 ns(1); ns <= max_spans; ++ns) {
			u64 const k((NB + ns - 1) / ns), spans((NB + k - 1) / k), wgs(P * spans);
			double const score(double(wgs) / double((wgs + n_cus - 1) / n_cus * n_cus) * double(k) / double(k + 1));
			if (score > best * 1.005) { best = score; span_blocks = k; }
		}
	}
	if (0 == span_blocks) {
		if (NB <= 32 && P >= 1024) span_blocks = NB;
		else {
			span_blocks = 32;
			while (span_blocks > 4 && P * ((NB + span_blocks - 1) / span_blocks) < 1024) span_blocks /= 2;
		}
	}
	u64 const NS((NB + span_blocks - 1) / span_blocks);
	xcd_grid g;
	if (P > 0xFFFFFFFFull || NS > 0xFFFFFFFFull || span_blocks > 0xFFFFull || SP >= (u64(1) << 23) || 4 * DP + DW >= (u64(1) << 29) || !make_xcd_grid(P * NS, xcd, g))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "matrix too large for one transpose launch");
	{
		timed_launch tl(ctx, V2M_KERNEL_TRANSPOSE);
		u32 const panel_fastest(1 == order ? 1u : 2 == order ? 0u : 1u);
		// whole SHORT columns of a dense destination whose columns do not start on lines: every line written once, by the column it
		// begins in.  (Short: the column ends are 2 of 6 lines at config 3's 79 words, where this is worth 9 %; at config 5's 313
		// words they are 2 of 21 and the 34 registers the kernel needs for it cost more than they bring.)
		if (kMayMerge && 1 == NS && NB <= 8 && DP == DW && DW >= 16 && 0 != DP % 16)
			hipLaunchKernelGGL((v2m::transpose_bits_lines_kernel<kWaves, kDepth, kTsR, kSlabRows, kMayMerge>), dim3(g.blocks), dim3(64 * kWaves), 0, ctx->stream,
				d_src, d_dst, SW, DW, SP, DP, u32(P), u32(NS), u32(span_blocks), g.items_per_xcd, panel_fastest);
		else
			hipLaunchKernelGGL((v2m::transpose_bits_lines_kernel<kWaves, kDepth, kTsR, kSlabRows, false>), dim3(g.blocks), dim3(64 * kWaves), 0, ctx->stream,
				d_src, d_dst, SW, DW, SP, DP, u32(P), u32(NS), u32(span_blocks), g.items_per_xcd, panel_fastest);
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}

#ifdef V2M_TUNING_BUILD
// The rotating-line kernel (tuning build only: it lost): kTsR row-words per workgroup on kWaves waves, spans of `span_blocks` blocks of 16 column groups (0: chosen here:
// the longest of 32 / 16 / 8 / 4 blocks that still leaves 2048 workgroups -- with ~80 VGPRs three workgroups of 8 waves share a CU).
template <int kWaves, int kDepth, int kTsR>
int launch_transpose_rot(v2m_ctx *ctx, u64 const *d_src, u64 SW, u64 DW, u64 SP, u64 DP, u64 *d_dst, u64 span_blocks, bool xcd, int order)
{
	u64 const P((SW + kTsR - 1) / kTsR), NB((DW + 15) / 16);
	if (0 == span_blocks) {
		span_blocks = 32;
		while (span_blocks > 4 && P * ((NB + span_blocks - 1) / span_blocks) < 2048) span_blocks /= 2;
	}
	u64 const NS((NB + span_blocks - 1) / span_blocks);
	xcd_grid g;
	if (P > 0xFFFFFFFFull || NS > 0xFFFFFFFFull || span_blocks > 0xFFFFull || SP >= (u64(1) << 23) || DW >= (u64(1) << 28) || !make_xcd_grid(P * NS, xcd, g))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "matrix too large for one transpose launch");
	{
		timed_launch tl(ctx, V2M_KERNEL_TRANSPOSE);
		u32 const panel_fastest(1 == order ? 1u : 2 == order ? 0u : 1u);
		hipLaunchKernelGGL((v2m::transpose_bits_rot_kernel<kWaves, kDepth, kTsR>), dim3(g.blocks), dim3(64 * kWaves), 0, ctx->stream,
			d_src, d_dst, SW, DW, SP, DP, u32(P), u32(NS), u32(span_blocks), g.items_per_xcd, panel_fastest);
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}
#endif   // V2M_TUNING_BUILD

// Kernel names: "8x8", "4x16", ... (LDS panel kR x kC), "stream16", "lines8[:K]" / "lines16[:K]" (whole lines, 8 / 16 row-words per workgroup, spans of K blocks), "ring:R,W,S,D[,K[,slow|nt]]" (tuning build; slow = ds_bpermute
// butterfly, nt = nontemporal loads and stores); trailing "/rr" keeps the plain round-robin dispatch order instead of XCD chunks, "/pf" / "/sf" make the row
// panels / the column panels (spans) run fastest in item order instead of the shorter dimension.
#ifdef V2M_TUNING_BUILD
constexpr bool kTuningBuild = true;
#else
constexpr bool kTuningBuild = false;
#endif

int launch_transpose_named(v2m_ctx *ctx, std::string shape, u64 const *d_src, u64 SW, u64 DW, u64 SP, u64 DP, u64 *d_dst)
{
	bool xcd(true);
	int order(0);
	for (bool again(true); again && shape.size() > 3;) {
		std::string const tail(shape.substr(shape.size() - 3));
		again = true;
		if (tail == "/rr") xcd = false;
		else if (tail == "/pf") order = 1;
		else if (tail == "/sf") order = 2;
		else again = false;
		if (again) shape.resize(shape.size() - 3);
	}
	if (0 == shape.compare(0, 5, "ring:")) {
		int R(0), W(0), S(0), D(0), K(0);
		char tail[16] = "";
		int const got(std::sscanf(shape.c_str() + 5, "%d,%d,%d,%d,%d,%15s", &R, &W, &S, &D, &K, tail));
		if (got < 4) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad transpose kernel name '%s'", shape.c_str());
		[[maybe_unused]] bool const fast(0 != std::strcmp(tail, "slow")), nt(0 == std::strcmp(tail, "nt"));
		// The product build holds the kernels the library picks among (kTransposeCandidates): 8x8, stream16, lines8 and lines16.  The other
		// shapes and flavours measured on the way there (tools/tune_transpose.py) are compiled with -DV2M_TUNING_BUILD
		// only (vcf2multialign_amd/libv2m_hip_tuning.so, loaded with V2M_HIP_LIBRARY by the tuning tool and the variant tests).
#define V2M_RING_FLAVOUR(r, w, s, d, f, n) launch_transpose_ring<r, w, s, d, f, n>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order)
#ifdef V2M_TUNING_BUILD
#define V2M_RING(r, w, s, d)                                                                                         \
		if (R == r && W == w && S == s && D == d)                                                                    \
			return !fast ? V2M_RING_FLAVOUR(r, w, s, d, false, false) : nt ? V2M_RING_FLAVOUR(r, w, s, d, true, true) : V2M_RING_FLAVOUR(r, w, s, d, true, false);
		V2M_RING(16, 8, 8, 4) V2M_RING(16, 16, 8, 8) V2M_RING(16, 8, 4, 4) V2M_RING(16, 8, 16, 4)
		V2M_RING(8, 4, 8, 4) V2M_RING(8, 4, 8, 8) V2M_RING(8, 8, 8, 4) V2M_RING(8, 8, 8, 8) V2M_RING(8, 8, 8, 16)
		V2M_RING(16, 16, 16, 8) V2M_RING(8, 8, 16, 8)   // (round 5: whole-line sectors with the lean butterfly; profiles/r05/transpose_rot8_experiment.txt)
#undef V2M_RING
#endif
#undef V2M_RING_FLAVOUR
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "transpose kernel '%s' is not in this build%s", shape.c_str(), kTuningBuild ? "" : " (the product build has 8x8, stream16, lines8 and lines16; the rest needs -DV2M_TUNING_BUILD)");
	}
	if (shape == "stream16") return launch_transpose_stream<4, 64>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
#ifdef V2M_TUNING_BUILD
	if (0 == shape.compare(0, 4, "rot8")) {
		// "rot8[:K[,V]]": spans of K blocks (0 / absent = chosen per shape); V = geometry variant
		int K(0), V(8);
		if (shape.size() > 4 && (':' != shape[4] || std::sscanf(shape.c_str() + 5, "%d,%d", &K, &V) < 1 || K < 0)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad transpose kernel name '%s'", shape.c_str());
		if (8 == V) return launch_transpose_rot<8, 4, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);
		if (88 == V) return launch_transpose_rot<8, 8, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);            // 8 steps of prefetch
		if (4 == V) return launch_transpose_rot<4, 4, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);             // 4 waves, two tiles each
		if (16 == V) return launch_transpose_rot<8, 4, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);           // 16 row-words (128-B source runs), two tiles per wave
		if (1616 == V) return launch_transpose_rot<16, 4, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);        // 16 row-words on 16 waves
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad transpose kernel name '%s'", shape.c_str());
	}
#endif
	if (0 == shape.compare(0, 7, "lines16")) {
		// "lines16[:K]": the whole-line kernel with 16 row-words per workgroup (128-byte source runs) on 8 waves, two tiles each; spans of K blocks (0 / absent = chosen per shape)
		int K(0);
		if (shape.size() > 7 && (':' != shape[7] || std::sscanf(shape.c_str() + 8, "%d", &K) < 1 || K < 0)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad transpose kernel name '%s'", shape.c_str());
		return launch_transpose_lines<8, 4, 16, 32, true>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);
	}
	if (0 == shape.compare(0, 6, "lines8")) {
		// "lines8[:K]": spans of K blocks (0 / absent = chosen per shape); the tuning build also has "lines8:K,V" with V = another geometry
		int K(0), V(8);
		if (shape.size() > 6 && (':' != shape[6] || std::sscanf(shape.c_str() + 7, "%d,%d", &K, &V) < 1 || K < 0)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad transpose kernel name '%s'", shape.c_str());
		if (8 == V) return launch_transpose_lines<8, 4, 8, 32, true>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);
#ifdef V2M_TUNING_BUILD
		if (4 == V) return launch_transpose_lines<4, 4>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);                // 4 waves, two tiles each
		if (88 == V) return launch_transpose_lines<8, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);               // 8 steps of prefetch
		if (816 == V) return launch_transpose_lines<8, 4, 8, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);       // 16-column slab
		if (16 == V) return launch_transpose_lines<16, 4, 16, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);      // 16 row-words on 16 waves
		if (168 == V) return launch_transpose_lines<16, 8, 16, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);
		if (1 == V) return launch_transpose_lines<8, 4>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);                // the product's geometry without the merged column ends
		if (28 == V) return launch_transpose_lines<8, 4, 16, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);       // 16 row-words (128-B source runs) on 8 waves, two tiles each (round 5, late: profiles/r05/transpose_pmc.txt)
		if (281 == V) return launch_transpose_lines<8, 4, 16, 32, true>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);  // the same, merged column ends where they apply
		if (288 == V) return launch_transpose_lines<8, 8, 16, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);      // the same with 8 steps of prefetch
		if (282 == V) return launch_transpose_lines<8, 2, 16, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);      // the same with 2 steps of prefetch
		if (2816 == V) return launch_transpose_lines<8, 4, 16, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, u64(K), xcd, order);     // the same with a 16-column slab
#endif
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "transpose kernel '%s' is not in this build%s", shape.c_str(), kTuningBuild ? "" : " (needs -DV2M_TUNING_BUILD)");
	}
#ifdef V2M_TUNING_BUILD
	if (shape == "stream16:old") return launch_transpose_stream<4, 64, 4, 16, 16, false>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:2,64") return launch_transpose_stream<2, 64>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:4,32") return launch_transpose_stream<4, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:2,32") return launch_transpose_stream<2, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:3,32") return launch_transpose_stream<3, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:2,16") return launch_transpose_stream<2, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:4,32,8") return launch_transpose_stream<4, 32, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:4,16,8") return launch_transpose_stream<4, 16, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:2,16,8") return launch_transpose_stream<2, 16, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream16:4,64,8") return launch_transpose_stream<4, 64, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream8x32") return launch_transpose_stream<4, 32, 4, 8, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream8x32:8") return launch_transpose_stream<4, 16, 8, 8, 32>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream32x8") return launch_transpose_stream<4, 64, 4, 32, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "stream4x64") return launch_transpose_stream<4, 16, 4, 4, 64>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
#endif
	if (shape == "8x8") return launch_transpose_shape<8, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
#ifdef V2M_TUNING_BUILD
	if (shape == "4x16") return launch_transpose_shape<4, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "16x8") return launch_transpose_shape<16, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "16x4") return launch_transpose_shape<16, 4>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "4x8") return launch_transpose_shape<4, 8>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "8x4") return launch_transpose_shape<8, 4>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
	if (shape == "8x16") return launch_transpose_shape<8, 16>(ctx, d_src, SW, DW, SP, DP, d_dst, xcd, order);
#endif
	return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "unknown transpose kernel '%s'", shape.c_str());
}

// Several kernels implement the transpose; which is fastest depends on the matrix shape, so matrices of at least 32 MiB
// are timed once per shape and context with each candidate (the result is the same either way) and the fastest is
// remembered.  V2M_TRANSPOSE_PANEL forces one; V2M_TRANSPOSE_CANDIDATES (comma-free list separated by ';') replaces the list.
char const *const kTransposeCandidates[] = {"8x8", "stream16", "lines8", "lines16"};

// src_pitch / dst_pitch: words from one column to the next (0 = dense: n_rows / 64 and n_cols / 64).
int launch_transpose(v2m_ctx *ctx, u64 const *d_src, u64 n_rows, u64 n_cols, u64 *d_dst, u64 src_pitch = 0, u64 dst_pitch = 0)
{
	u64 const SW(n_rows / 64), DW(n_cols / 64);
	u64 const SP(src_pitch ? src_pitch : SW), DP(dst_pitch ? dst_pitch : DW);
	char const *e(std::getenv("V2M_TRANSPOSE_PANEL"));
	if (e && *e) return launch_transpose_named(ctx, e, d_src, SW, DW, SP, DP, d_dst);
	if (SW * DW * 512 < (u64(32) << 20)) return launch_transpose_named(ctx, "8x8", d_src, SW, DW, SP, DP, d_dst);
	for (auto const &c : ctx->transpose_choice)
		if (c.rows == n_rows && c.cols == n_cols && c.src_pitch == SP && c.dst_pitch == DP) return launch_transpose_named(ctx, c.kernel, d_src, SW, DW, SP, DP, d_dst);

	std::vector<std::string> names;
	if (char const *list = std::getenv("V2M_TRANSPOSE_CANDIDATES")) {
		std::string cur;
		for (char const *p(list); ; ++p) {
			if (';' == *p || 0 == *p) { if (!cur.empty()) names.push_back(cur); cur.clear(); if (0 == *p) break; }
			else cur.push_back(*p);
		}
	}
	if (names.empty()) names.assign(std::begin(kTransposeCandidates), std::end(kTransposeCandidates));

	std::vector<float> best(names.size(), 1e30f);
	{
		scoped_events ev;
		V2M_HIP_TRY(ctx, ev.create(names.size() + 1));
		scoped_profiling_off const quiet(ctx);   // the calibration launches are not the caller's
		std::vector<char> usable(names.size(), 1);   // a candidate may decline a shape (its index arithmetic is 32-bit): it is left out, not an error
		for (int rep(0); rep < 3; ++rep) {        // the first round touches the pages; the better of the next two counts (one timing alone picked the wrong kernel now and then: the candidates are within 10 % of each other and a launch's time depends on what the one before it left in the caches)
			V2M_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
			for (std::size_t k(0); k < names.size(); ++k) {
				if (usable[k]) {
					int const rc(launch_transpose_named(ctx, names[k], d_src, SW, DW, SP, DP, d_dst));
					if (V2M_ERR_UNSUPPORTED == rc) usable[k] = 0;
					else if (rc) return rc;
				}
				V2M_HIP_TRY(ctx, hipEventRecord(ev[k + 1], ctx->stream));
			}
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			for (std::size_t k(0); k < names.size(); ++k) {
				float ms(0);
				V2M_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
				if (rep && usable[k]) best[k] = std::min(best[k], ms);
			}
		}
		if (std::none_of(usable.begin(), usable.end(), [](char u) { return 0 != u; })) return fail(ctx, V2M_ERR_UNSUPPORTED, "matrix too large for one transpose launch");
		if (std::any_of(usable.begin(), usable.end(), [](char u) { return 0 == u; })) ctx->err.clear();   // (the declining candidate's message)
	}
	std::size_t const pick(std::size_t(std::min_element(best.begin(), best.end()) - best.begin()));
	ctx->transpose_choice.push_back({n_rows, n_cols, SP, DP, names[pick]});
	std::string note("transpose " + std::to_string(n_rows) + "x" + std::to_string(n_cols) + " bits" + ((SP != SW || DP != DW) ? " (column pitches " + std::to_string(SP) + " / " + std::to_string(DP) + " words)" : std::string()) + ": " + names[pick] + " (");
	for (std::size_t k(0); k < names.size(); ++k) {
		char buf[64];
		std::snprintf(buf, sizeof(buf), "%s%s %.3f ms", k ? ", " : "", names[k].c_str(), best[k]);
		note += buf;
	}
	note += ")";
	if (ctx->info.size() > 2000) ctx->info.clear();
	if (!ctx->info.empty()) ctx->info += "; ";
	ctx->info += note;
	// the calibration already produced the result; run the chosen kernel once more under the caller's profiling so
	// that its launch is accounted for like any other
	return launch_transpose_named(ctx, names[pick], d_src, SW, DW, SP, DP, d_dst);
}


// Host-side preparation of a row batch: validates it against the uploaded graph and flattens
// every row into (edge_begin, copy) segments.  The tables are written straight into the context's pinned
// staging area: founder batches carry hundreds of thousands of segments per row, and uploading those from pageable
// memory makes the runtime pin and unpin the pages as userptr memory, which stalls the queue for tens of ms.
struct prepared_rows {
	u32 *seg_offsets{};      // [n_rows + 1]
	u32 *seg_edge_begin{};   // [n_segments]
	u32 *seg_copy{};         // [n_segments]
	u64 n_rows{}, n_segments{};
	bool any_switching_row{};
};

int prepare_rows(v2m_ctx *ctx, v2m_row_batch const *rows, u64 row_begin, u64 row_end, prepared_rows &out)
{
	u64 const n_rows(row_end - row_begin);
	u64 max_segments(n_rows);                                 // a row without cuts is one segment ...
	if (rows->cut_offsets) {
		for (u64 r(row_begin); r < row_end; ++r) {
			if (rows->cut_offsets[r + 1] < rows->cut_offsets[r])
				return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "cut_offsets decrease at row %llu", (unsigned long long) r);
			max_segments += rows->cut_offsets[r + 1] - rows->cut_offsets[r];   // ... one with cuts has one per cut, plus a leading REF one
		}
	}
	if (max_segments >= 0xFFFFFFFFull)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "row batch has too many cut segments (%llu) for one call", (unsigned long long) max_segments);
	auto const pad([](u64 n) { return (n * sizeof(u32) + 63) & ~u64(63); });
	int const area(ctx->row_stage_next);
	if (ctx->row_stage_in_flight[area]) {
		V2M_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_row_stage[area]));   // the uploads of two slices ago
		ctx->row_stage_in_flight[area] = false;
	}
	V2M_HIP_TRY(ctx, ctx->h_row_stage[area].ensure(pad(n_rows + 1) + 2 * pad(max_segments)));
	char *const base(static_cast<char *>(ctx->h_row_stage[area].p));
	V2M_POISON_HOST(base, pad(n_rows + 1) + 2 * pad(max_segments));
	out.seg_offsets = reinterpret_cast<u32 *>(base);
	out.seg_edge_begin = reinterpret_cast<u32 *>(base + pad(n_rows + 1));
	out.seg_copy = reinterpret_cast<u32 *>(base + pad(n_rows + 1) + pad(max_segments));
	out.n_rows = n_rows;
	out.any_switching_row = false;

	// segment offsets first (a row with cuts: one segment per cut, plus a leading REF one unless its first cut is node 0), then the
	// rows are filled independently of each other: founder batches carry hundreds of thousands of cuts per row (config 4: 672 495 x 26
	// rows, each cut checked against the graph), which a few threads do in a quarter of the time
	out.seg_offsets[0] = 0;
	for (u64 r(row_begin); r < row_end; ++r) {
		u64 const c_begin(rows->cut_offsets ? rows->cut_offsets[r] : 0), c_end(rows->cut_offsets ? rows->cut_offsets[r + 1] : 0);
		u64 const n_seg(c_begin == c_end ? 1 : (c_end - c_begin) + (0 != rows->cut_nodes[c_begin] ? 1 : 0));
		out.seg_offsets[r - row_begin + 1] = u32(out.seg_offsets[r - row_begin] + n_seg);
		out.any_switching_row = out.any_switching_row || n_seg > 1;
	}
	out.n_segments = out.seg_offsets[n_rows];

	// (error messages are composed where the error is found; the first failing row in row order is the one reported)
	struct row_error { int code{V2M_OK}; std::string text; };
	auto const fill_row([&](u64 r, row_error &err) {
		auto const failed([&](int code, char const *fmt, unsigned long long a, unsigned long long b = 0) {
			char buf[256];
			std::snprintf(buf, sizeof(buf), fmt, a, b);
			err.code = code;
			err.text = buf;
		});
		u64 const c_begin(rows->cut_offsets ? rows->cut_offsets[r] : 0), c_end(rows->cut_offsets ? rows->cut_offsets[r + 1] : 0);
		u32 n(out.seg_offsets[r - row_begin]);
		if (c_begin == c_end) {
			if (!rows->copy_index) return failed(V2M_ERR_INVALID_ARGUMENT, "row %llu has no cuts and rows->copy_index is NULL", r);
			u32 const copy(rows->copy_index[r]);
			if (copy != V2M_PLOIDY_MAX && (!ctx->d_paths || copy >= ctx->path_cols))
				return failed(V2M_ERR_INVALID_ARGUMENT, "row %llu: chromosome copy %llu is outside the path matrix", r, copy);
			out.seg_edge_begin[n] = 0;
			out.seg_copy[n] = copy;
			return;
		}
		u64 prev(0);
		for (u64 k(c_begin); k < c_end; ++k) {
			u64 const node(rows->cut_nodes[k]);
			u32 const copy(rows->cut_copies[k]);
			if (node >= ctx->n_nodes) return failed(V2M_ERR_PRECONDITION, "row %llu: cut node %llu does not exist", r, node);
			if (k > c_begin && node <= prev) return failed(V2M_ERR_PRECONDITION, "row %llu: cut nodes must be strictly increasing", r);
			if (copy != V2M_PLOIDY_MAX && (!ctx->d_paths || copy >= ctx->path_cols))
				return failed(V2M_ERR_INVALID_ARGUMENT, "row %llu: chromosome copy %llu is outside the path matrix", r, copy);
			u32 const first_edge(ctx->h_csum[node]);
			// founder_sequence_greedy_output.cc:108 asserts the walk never jumps over a cut node
			if (node > 0 && ctx->h_tgt_prefix_max[first_edge] > node)
				return failed(V2M_ERR_PRECONDITION, "row %llu: cut node %llu lies inside the span of an ALT edge", r, node);
			if (k == c_begin && node != 0) {   // copy index is PLOIDY_MAX until the first cut is visited
				out.seg_edge_begin[n] = 0;
				out.seg_copy[n] = V2M_PLOIDY_MAX;
				++n;
			}
			out.seg_edge_begin[n] = first_edge;
			out.seg_copy[n] = copy;
			++n;
			prev = node;
		}
	});
	std::vector<row_error> errors(n_rows);
	unsigned const n_threads(out.n_segments >= (u64(1) << 20) ? unsigned(std::min<u64>(n_rows, 8)) : 1u);
	if (n_threads <= 1) {
		for (u64 r(row_begin); r < row_end; ++r) { fill_row(r, errors[r - row_begin]); if (V2M_OK != errors[r - row_begin].code) break; }
	}
	else {
		std::atomic<u64> next(row_begin);
		auto const work([&] { for (u64 r; (r = next.fetch_add(1)) < row_end;) fill_row(r, errors[r - row_begin]); });
		std::vector<std::thread> pool;
		for (unsigned t(1); t < n_threads; ++t) pool.emplace_back(work);
		work();
		for (auto &t : pool) t.join();
	}
	for (auto const &e : errors) if (V2M_OK != e.code) return fail(ctx, e.code, "%s", e.text.c_str());
	return V2M_OK;
}


// Tuning knobs (read per call so that one process can A/B them).
// V2M_NT_STORES=0/1 (aligned) and V2M_UNALIGNED_STORE=plain|nt (unaligned) force plain / nontemporal output stores; unset = calibrate
// once per context (store_flavour_launch).  -1 = not forced.
int forced_store_mode(bool unaligned)
{
	if (unaligned) {
		char const *const e = std::getenv("V2M_UNALIGNED_STORE");
		if (e && 0 == std::strcmp(e, "plain")) return 0;
		if (e && 0 == std::strcmp(e, "nt")) return 1;
		return -1;
	}
	char const *e = std::getenv("V2M_NT_STORES");
	if (!(e && *e)) return -1;
	return std::atoi(e) != 0 ? 1 : 0;
}

u32 rows_per_group_for(u64 n_rows)
{
	char const *e = std::getenv("V2M_ROWS_PER_GROUP");
	int const v((e && *e) ? std::atoi(e) : 0);
	if (v > 0) return u32(std::min(v, 256));   // count_unaligned_kernel holds at most 256 rows per group
	// 32 rows per workgroup: the template tile and the patch cache are set up once per group (a prologue of dependent L2 / HBM round trips during which
	// the workgroup stores nothing) and the effective-edge words are reloaded every 16 rows (kGroupRowsLds).  Measured per 620 rows of config 3 /
	// 244 of config 5 on one box (profiles/r05/rows_per_group.txt): 16 rows 9.39-9.57 / 9.07-9.35 ms (unaligned 10.65-10.84 / 11.0-11.7), 32 rows
	// 9.06-9.32 / 9.14-9.31 (10.16-10.30 / 10.9-11.6), 48 rows 9.31-9.51 / 9.20-9.42, 64 rows 9.12-9.33 / 9.35-9.44.
	return u32(std::min<u64>(32, std::max<u64>(1, n_rows)));
}


// Rows per workgroup over the tiles of a window set.  A workgroup pays its prologue (the tile tables, load_patch_cache, the first effective-
// edge words: a chain of dependent L2 / HBM round trips) once per group whatever the tile's length, and a 300-byte tile gives it next to
// nothing to store per row.  So a group takes as many rows as keep the bytes it writes at what 32 rows of a full tile come to
// (32 * kTileBytes / mean tile length), up to the 256 rows the count kernel holds (V2M_ROWS_PER_GROUP's ceiling as well).  A guess
// until measured.  V2M_ROWS_PER_GROUP overrides it as everywhere.
u32 rows_per_group_for_set(u64 n_rows, u64 mean_tile_bytes)
{
	char const *e = std::getenv("V2M_ROWS_PER_GROUP");
	if (e && *e && std::atoi(e) > 0) return rows_per_group_for(n_rows);
	u64 const by_bytes(32 * u64(v2m::kTileBytes) / std::max<u64>(1, mean_tile_bytes));
	return u32(std::min<u64>(std::max<u64>(1, n_rows), std::min<u64>(256, std::max<u64>(32, by_bytes))));
}


// The REF row of a view with `gap` as padding ('-', or 0 for the unaligned kernels) into dst: chunk c holds columns view.begin + 16 c on.
int expand_reference(v2m_ctx *ctx, row_view const &v, dev_buf &dst, char gap)
{
	u64 const n_chunks(u64(v.n_tiles) * v2m::kTileChunks);
	V2M_HIP_TRY(ctx, dst.ensure(n_chunks * 16));
	{
		timed_launch tl(ctx, V2M_KERNEL_TEMPLATE);
		hipLaunchKernelGGL(v2m::expand_reference_row_kernel, dim3(unsigned((n_chunks + 255) / 256)), dim3(256), 0, ctx->stream,
			ctx->d_ref.as<char>(), ctx->d_ref_pos.as<u32>(), ctx->d_aln_pos.as<u32>(), u32(ctx->n_nodes), u32(v.end), n_chunks, dst.as<uint4>(), gap, u32(v.begin));
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}


// Effective-edge bits of rows [row_begin, row_end) of the batch into ctx->d_eff (the words of the view in force, laid out as its word_range says).
int resolve_slice(v2m_ctx *ctx, v2m_row_batch const *rows, u64 row_begin, u64 row_end)
{
	u64 const n_rows(row_end - row_begin);
	word_range const wr(ctx->view().words);
	u64 const eff_words(wr.stride), n_words(wr.hi);   // words [wr.lo, n_words) are resolved
	if (0 == ctx->n_edges) return V2M_OK;

	prepared_rows pr;
	if (int const rc = prepare_rows(ctx, rows, row_begin, row_end, pr)) return rc;
	if (wr.lo >= wr.hi) return V2M_OK;   // a column window that no edge reaches into
	auto const upload([&](scratch_buf &dst, u32 const *src, u64 count) -> int {
		V2M_HIP_TRY(ctx, dst.ensure(std::max<size_t>(count * sizeof(u32), 16)));
		if (count) V2M_HIP_TRY(ctx, hipMemcpyAsync(dst.p, src, count * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
		return V2M_OK;
	});
	// The staging area the tables came from is free again once these copies have run; the other one takes the next slice.  The
	// area counts as in flight from the first copy on, whether or not all three get queued: a failed call must not leave
	// copies behind that the next user of the area does not wait for.
	int const stage(ctx->row_stage_next);
	ctx->row_stage_in_flight[stage] = true;
	ctx->row_stage_next ^= 1;
	int upload_rc(upload(ctx->d_seg_offsets, pr.seg_offsets, n_rows + 1));
	if (!upload_rc) upload_rc = upload(ctx->d_seg_edge_begin, pr.seg_edge_begin, pr.n_segments);
	if (!upload_rc) upload_rc = upload(ctx->d_seg_copy, pr.seg_copy, pr.n_segments);
	hipError_t const recorded(hipEventRecord(ctx->ev_row_stage[stage], ctx->stream));
	if (upload_rc) return upload_rc;
	V2M_HIP_TRY(ctx, recorded);
	V2M_HIP_TRY(ctx, ctx->d_eff.ensure(n_rows * eff_words * sizeof(u64)));
	V2M_HIP_TRY(ctx, ctx->d_needs_serial.ensure(n_rows * sizeof(u32)));
	V2M_HIP_TRY(ctx, hipMemsetAsync(ctx->d_needs_serial.p, 0, n_rows * sizeof(u32), ctx->stream));

	// rows that switch copies (founder rows) get their bit column put together first
	bool const any_switching_row(pr.any_switching_row);
	if (any_switching_row) V2M_HIP_TRY(ctx, ctx->d_row_bits.ensure(n_rows * eff_words * sizeof(u64)));

	// (the scratch pointers are offset so that the kernels index them with edge words of the whole graph)
	u64 *const d_eff(ctx->d_eff.as<u64>() - wr.restart);
	u64 *const d_row_bits(any_switching_row ? ctx->d_row_bits.as<u64>() - wr.restart : nullptr);
	v2m::row_segments rs{ctx->d_seg_offsets.as<u32>(), ctx->d_seg_edge_begin.as<u32>(), ctx->d_seg_copy.as<u32>(), d_row_bits, u32(eff_words)};
	char const *const back_env(std::getenv("V2M_MAX_BACK_WORDS"));   // test knob: 0 forces the serial kernel for every cross-word restart
	u32 const max_back_words((back_env && *back_env) ? u32(std::strtoul(back_env, nullptr, 10)) : v2m::kMaxBackWords);
	char const *const capacity_env(std::getenv("V2M_RESOLVE_QUEUE_CAPACITY"));   // test knob: entries per queue shard, no floor (0: every hard word is decided in the streaming pass)
	bool const capacity_forced(capacity_env && *capacity_env);
	{
		timed_launch tl(ctx, V2M_KERNEL_RESOLVE);
		// rows per launch: queue entries are 32-bit (row, word) indices
		u64 const rows_per_launch(std::max<u64>(1, std::min<u64>(65535, 0xFFFFFFFFull / std::max<u64>(1, n_words))));
		u64 const assembled_words(n_words - wr.restart), resolved_words(n_words - wr.lo);
		for (u64 r0(0); r0 < n_rows; r0 += rows_per_launch) {
			u64 const nr(std::min<u64>(rows_per_launch, n_rows - r0));
			if (any_switching_row)
				for (u64 y0(0); y0 < nr; y0 += 65535)   // grid.y limit
					hipLaunchKernelGGL(v2m::assemble_row_bits_kernel, dim3(unsigned((assembled_words + 255) / 256), unsigned(std::min<u64>(65535, nr - y0))), dim3(256), 0, ctx->stream,
						ctx->d_paths, ctx->path_pitch, rs, d_row_bits, u32(n_words), u32(r0 + y0), u32(wr.restart));
			// the queue's segments hold every word of the launch if they have to (iid random bits do that), up to 1 GiB in all;
			// a workgroup whose segment is full decides its overflow itself
			u64 const shard_capacity(capacity_forced ? std::min<u64>(std::strtoull(capacity_env, nullptr, 10), (u64(1) << 28) / v2m::kResolveQueueShards)
				: std::max<u64>(256, std::min<u64>(nr * resolved_words, u64(1) << 28) / v2m::kResolveQueueShards));
			V2M_HIP_TRY(ctx, ctx->d_resolve_queue.ensure(shard_capacity * v2m::kResolveQueueShards * sizeof(u32)));
			V2M_HIP_TRY(ctx, ctx->d_resolve_count.ensure(v2m::kResolveQueueShards * sizeof(u32)));
			V2M_HIP_TRY(ctx, hipMemsetAsync(ctx->d_resolve_count.p, 0, v2m::kResolveQueueShards * sizeof(u32), ctx->stream));
			for (u64 piece0(0), pieces((resolved_words + 256 * v2m::kResolveWordsPerThread - 1) / (256 * v2m::kResolveWordsPerThread)); piece0 < pieces; piece0 += 65535)   // grid.y limit; rows run fastest
				hipLaunchKernelGGL(v2m::resolve_effective_edges_kernel, dim3(unsigned(nr), unsigned(std::min<u64>(65535, pieces - piece0))), dim3(256), 0, ctx->stream,
					ctx->d_paths, ctx->path_pitch, u32(ctx->n_edges), rs, ctx->d_spans.as<v2m::edge_span>(), ctx->d_overlappable.as<u64>(),
					ctx->d_ovl_rank.as<u32>(), ctx->d_blocker_masks.as<u64>(),
					d_eff, u32(n_words), u32(eff_words), u32(r0), u32(wr.lo + piece0 * 256 * v2m::kResolveWordsPerThread),
					ctx->d_resolve_queue.as<u32>(), ctx->d_resolve_count.as<u32>(), u32(shard_capacity), ctx->d_needs_serial.as<u32>(), max_back_words);
			hipLaunchKernelGGL(v2m::resolve_queued_words_kernel, dim3(2 * v2m::kResolveQueueShards), dim3(256), 0, ctx->stream,
				ctx->d_paths, ctx->path_pitch, u32(ctx->n_edges), rs, ctx->d_spans.as<v2m::edge_span>(), ctx->d_overlappable.as<u64>(),
				d_eff, u32(n_words), u32(eff_words), u32(r0),
				ctx->d_resolve_queue.as<u32>(), ctx->d_resolve_count.as<u32>(), u32(shard_capacity), ctx->d_needs_serial.as<u32>(), max_back_words);
		}
		// rows whose restart point is too far back for the per-word kernel (chromosome-scale deletions)
		hipLaunchKernelGGL(v2m::resolve_rows_serial_kernel, dim3(unsigned((n_rows + 3) / 4)), dim3(256), 0, ctx->stream,
			ctx->d_paths, ctx->path_pitch, u32(ctx->n_edges), rs, ctx->d_spans.as<v2m::edge_span>(),
			d_eff, eff_words, u32(n_rows), ctx->d_needs_serial.as<u32>(), u32(wr.restart), u32(n_words));
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}


struct splice_grid {
	u32 rows_per_group, n_groups, tile_run;
	u64 n_blocks;
};

u32 tile_run_for(u32 n_tiles)
{
	char const *e = std::getenv("V2M_TILE_RUN");   // tuning knob
	int const v((e && *e) ? std::atoi(e) : 0);
	u32 const run(v > 0 ? u32(v) : 64u);
	return std::max<u32>(1, std::min(run, n_tiles));
}

int make_grid(v2m_ctx *ctx, u64 n_rows, splice_grid &g)
{
	g.rows_per_group = ctx->set_call ? rows_per_group_for_set(n_rows, ctx->set.mean_tile_bytes) : rows_per_group_for(n_rows);
	g.n_groups = u32((n_rows + g.rows_per_group - 1) / g.rows_per_group);
	g.n_blocks = u64(ctx->view().n_tiles) * g.n_groups;
	g.tile_run = tile_run_for(ctx->view().n_tiles);
	if (g.n_blocks > 0x7FFFFFFFull)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "splice grid too large (%llu workgroups); use smaller batches", (unsigned long long) g.n_blocks);
	return V2M_OK;
}


// Issues launch(nt) once more with the store flavour of the splice kind (ctx->store_mode, or ctx->unaligned_store_mode for the unaligned
// splice) and times it as that kind's kernel.  Output rows are written once and never re-read by the GPU, so nontemporal stores (which
// keep the rows from displacing the template and edge tables in L2 / Infinity Cache) usually win: 7.2-7.6 ms against 8.1-8.5 ms per
// 51-GB aligned launch at config 3.  But on some boxes / memory layouts they are stuck in a slower mode for the whole life of a process
// (9.1-9.3 ms, tools/probe_nt*.py), while plain stores stay put; the unaligned splice differs by box and buffer too (7.2 vs 5.4 ms per 256
// config-3 rows on one box, 5.6 vs 6.0 ms on another).  The flavour is therefore calibrated once per context and kind, on the first
// launch that writes >= 1 GiB (`bytes`): that launch is issued twice per flavour (the output is the same every time) and the faster one
// is kept.
template <typename F>
int store_flavour_launch(v2m_ctx *ctx, bool unaligned, u64 n_rows, u64 bytes, F const &launch)
{
	int &slot(unaligned ? ctx->unaligned_store_mode : ctx->store_mode);
	int mode(forced_store_mode(unaligned));
	if (mode < 0) mode = slot;
	if (mode < 0 && bytes >= (u64(1) << 30)) {
		scoped_events ev;
		V2M_HIP_TRY(ctx, ev.create(5));
		V2M_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
		for (int i(0); i < 4; ++i) {
			launch(0 == (i & 1));   // nt, plain, nt, plain
			V2M_HIP_TRY(ctx, hipEventRecord(ev[i + 1], ctx->stream));
		}
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		float t[4];
		for (int i(0); i < 4; ++i) V2M_HIP_TRY(ctx, hipEventElapsedTime(&t[i], ev[i], ev[i + 1]));
		float const nt_ms(std::min(t[0], t[2])), plain_ms(std::min(t[1], t[3]));
		slot = nt_ms <= plain_ms ? 1 : 0;
		char buf[160];
		std::snprintf(buf, sizeof(buf), "%s splice stores: %s (calibrated on %llu rows: nontemporal %.3f ms, plain %.3f ms)",
			unaligned ? "unaligned" : "aligned", slot ? "nontemporal" : "plain", (unsigned long long) n_rows, nt_ms, plain_ms);
		if (unaligned && ctx->info.size() > 2000) ctx->info.clear();
		if (!ctx->info.empty()) ctx->info += "; ";
		ctx->info += buf;
		mode = slot;
	}
	if (mode < 0) mode = 1;   // small launches before any calibration
	{
		timed_launch tl(ctx, unaligned ? V2M_KERNEL_SPLICE_UNALIGNED : V2M_KERNEL_SPLICE_ALIGNED);
		launch(0 != mode);
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}


v2m::set_tile_tables set_tables(v2m_ctx const *ctx)
{
	auto const &s(ctx->set);
	return {s.d_col_begin.as<u32>(), s.d_col_end.as<u32>(), s.d_record_offset.as<u32>(), s.d_edge_end.as<u32>()};
}

int expand_reference_set(v2m_ctx *ctx, dev_buf &dst, char gap);


// Resolve + aligned splice of rows [row_begin, row_end) of the batch into d_out.
int splice_aligned_slice(v2m_ctx *ctx, v2m_row_batch const *rows, u64 row_begin, u64 row_end, char *d_out, u64 row_pitch)
{
	u64 const n_rows(row_end - row_begin);
	if (0 == n_rows || 0 == ctx->aligned_len) return V2M_OK;
	if (int const rc = resolve_slice(ctx, rows, row_begin, row_end)) return rc;

	row_view const &v(ctx->view());
	splice_grid g;
	if (int const rc = make_grid(ctx, n_rows, g)) return rc;
	v2m::tile_tables const tt{v.d_edge_begin.as<u32>(), v.d_cross_offsets.as<u32>(), v.d_cross_edges.as<u32>()};
	u64 const store_limit((v.length() + 15) & ~u64(15));
	auto const launch([&](bool nt) {
		auto const go([&](auto kernel, auto... window) {
			hipLaunchKernelGGL(kernel, dim3(unsigned(g.n_blocks)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
				v.d_template.as<v2m::vec4u>(), ctx->d_eff.as<u64>() - v.words.restart, v.words.stride, tt, ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
				d_out, row_pitch, u32(n_rows), g.rows_per_group, g.n_groups, v.n_tiles, g.tile_run, store_limit, '-', window...);
		});
		if (ctx->set_call) {
			auto const go_set([&](auto kernel) {
				hipLaunchKernelGGL(kernel, dim3(unsigned(g.n_blocks)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
					v.d_template.as<v2m::vec4u>(), ctx->d_eff.as<u64>() - v.words.restart, v.words.stride, tt, set_tables(ctx), ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
					d_out, row_pitch, u32(n_rows), g.rows_per_group, g.n_groups, v.n_tiles, g.tile_run, '-');
			});
			if (nt) go_set(v2m::splice_aligned_set_kernel<true>);
			else go_set(v2m::splice_aligned_set_kernel<false>);
		}
		else if (ctx->windowed) {
			if (nt) go(v2m::splice_aligned_window_kernel<true>, u32(v.begin), u32(v.end));
			else go(v2m::splice_aligned_window_kernel<false>, u32(v.begin), u32(v.end));
		}
		else if (nt) go(v2m::splice_aligned_kernel<true>);
		else go(v2m::splice_aligned_kernel<false>);
	});
	return store_flavour_launch(ctx, false, n_rows, n_rows * v.length(), launch);
}


// Resolve + unaligned splice (count, scan, compact) of rows [row_begin, row_end) into d_out;
// leaves the row lengths in ctx->d_row_lengths.
int splice_unaligned_slice(v2m_ctx *ctx, v2m_row_batch const *rows, u64 row_begin, u64 row_end, char *d_out, u64 row_pitch)
{
	u64 const n_rows(row_end - row_begin);
	if (0 == n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, ctx->d_row_lengths.ensure(n_rows * sizeof(u64)));
	if (0 == ctx->aligned_len) {
		V2M_HIP_TRY(ctx, hipMemsetAsync(ctx->d_row_lengths.p, 0, n_rows * sizeof(u64), ctx->stream));
		return V2M_OK;
	}
	row_view &v(ctx->view());
	bool const set(ctx->set_call);
	if (!v.has_template0) {   // the REF row with 0 as padding, built on first use
		if (int const rc = set ? expand_reference_set(ctx, v.d_template0, 0) : expand_reference(ctx, v, v.d_template0, 0)) return rc;
		v.has_template0 = true;
	}
	if (int const rc = resolve_slice(ctx, rows, row_begin, row_end)) return rc;

	splice_grid g;
	if (int const rc = make_grid(ctx, n_rows, g)) return rc;
	V2M_HIP_TRY(ctx, ctx->d_tile_counts.ensure(n_rows * v.n_tiles * sizeof(u32)));
	if (set) {
		V2M_HIP_TRY(ctx, ctx->d_set_tile_offsets.ensure(n_rows * v.n_tiles * sizeof(u32)));
		V2M_HIP_TRY(ctx, ctx->d_set_lengths[ctx->set_lengths_slot].ensure(n_rows * ctx->set.n_windows * sizeof(u32)));
	}
	bool const windowed(ctx->windowed);
	v2m::tile_tables const tt{v.d_edge_begin.as<u32>(), v.d_cross_offsets.as<u32>(), v.d_cross_edges.as<u32>()};
	u64 const *const d_eff(ctx->d_eff.as<u64>() - v.words.restart);
	{
		// pass 1 builds no row, so it takes more rows per workgroup than pass 2 (the template tile, its byte count and the candidates' changes
		// are set up once per group): as many as the kernel holds (kCountRowsMax = 256; measured per 620 / 244 rows of config 3 / 5: 32 rows
		// 0.64 / 0.84 ms, 64 rows 0.48 / 0.64, 128 rows 0.41 / 0.53, 256 rows 0.38 / 0.49).  V2M_COUNT_ROWS_PER_GROUP overrides.
		char const *const ce(std::getenv("V2M_COUNT_ROWS_PER_GROUP"));
		u32 const count_rows(u32(std::min<u64>(std::max<u64>(1, n_rows), (ce && *ce && std::atoi(ce) > 0) ? u64(std::min(std::atoi(ce), int(v2m::kCountRowsMax))) : u64(v2m::kCountRowsMax))));
		u32 const count_groups(u32((n_rows + count_rows - 1) / count_rows));
		timed_launch tl(ctx, V2M_KERNEL_UNALIGNED_COUNT);
		auto const count([&](auto kernel, auto... window) {
			hipLaunchKernelGGL(kernel, dim3(unsigned(u64(v.n_tiles) * count_groups)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
				v.d_template0.as<v2m::vec4u>(), d_eff, v.words.stride, tt, ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
				ctx->d_tile_counts.as<u32>(), v.n_tiles, u32(n_rows), count_rows, count_groups, g.tile_run, window...);
		});
		if (set)
			hipLaunchKernelGGL(v2m::count_unaligned_set_kernel, dim3(unsigned(u64(v.n_tiles) * count_groups)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
				v.d_template0.as<v2m::vec4u>(), d_eff, v.words.stride, tt, set_tables(ctx), ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
				ctx->d_tile_counts.as<u32>(), v.n_tiles, u32(n_rows), count_rows, count_groups, g.tile_run);
		else if (windowed) count(v2m::count_unaligned_window_kernel, u32(v.begin), u32(v.end));
		else count(v2m::count_unaligned_kernel);
		hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(unsigned(n_rows)), dim3(256), 0, ctx->stream,
			ctx->d_tile_counts.as<u32>(), v.n_tiles, ctx->d_row_lengths.as<u64>());
		if (set)   // the scan segmented at each window's first tile: the tiles' destinations in the record, the pieces' lengths
			hipLaunchKernelGGL(v2m::scan_window_set_kernel, dim3(unsigned(n_rows)), dim3(256), 0, ctx->stream,
				ctx->d_tile_counts.as<u32>(), ctx->d_row_lengths.as<u64>(), v.n_tiles, u32(ctx->set.n_windows),
				ctx->set.d_first_tile.as<u32>(), ctx->set.d_tile_window.as<u32>(), ctx->set.d_slot_offset32.as<u32>(),
				ctx->d_set_tile_offsets.as<u32>(), ctx->d_set_lengths[ctx->set_lengths_slot].as<u32>());
	}
	auto const launch([&](bool nt) {
		auto const go([&](auto kernel, auto... window) {
			hipLaunchKernelGGL(kernel, dim3(unsigned(g.n_blocks)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
				v.d_template0.as<v2m::vec4u>(), d_eff, v.words.stride, tt, ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
				ctx->d_tile_counts.as<u32>(), v.n_tiles, d_out, row_pitch, u32(n_rows), g.rows_per_group, g.n_groups, g.tile_run, window...);
		});
		if (set) {
			auto const go_set([&](auto kernel) {
				hipLaunchKernelGGL(kernel, dim3(unsigned(g.n_blocks)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
					v.d_template0.as<v2m::vec4u>(), d_eff, v.words.stride, tt, set_tables(ctx), ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
					ctx->d_set_tile_offsets.as<u32>(), v.n_tiles, d_out, row_pitch, u32(n_rows), g.rows_per_group, g.n_groups, g.tile_run);
			});
			if (nt) go_set(v2m::splice_unaligned_set_kernel<true>);
			else go_set(v2m::splice_unaligned_set_kernel<false>);
			return;
		}
		if (windowed) {
			if (nt) go(v2m::splice_unaligned_window_kernel<true>, u32(v.begin), u32(v.end));
			else go(v2m::splice_unaligned_window_kernel<false>, u32(v.begin), u32(v.end));
			return;
		}
#ifdef V2M_TUNING_BUILD
		// V2M_UNALIGNED_KERNEL=wave | shared64: the stream-out whose every wave packs its own short chunks / the product's with a queue of 64 (tools/unaligned_ab.sh)
		static int const flavour([] { char const *const e(std::getenv("V2M_UNALIGNED_KERNEL")); return !e ? 0 : 0 == std::strcmp(e, "wave") ? 1 : 0 == std::strcmp(e, "shared64") ? 2 : 0; }());
		if (1 == flavour) { if (nt) go(v2m::splice_unaligned_per_wave_kernel<true>); else go(v2m::splice_unaligned_per_wave_kernel<false>); return; }
		if (2 == flavour) { if (nt) go(v2m::splice_unaligned_kernel<true, 64>); else go(v2m::splice_unaligned_kernel<false, 64>); return; }
#endif
		if (nt) go(v2m::splice_unaligned_kernel<true>);
		else go(v2m::splice_unaligned_kernel<false>);
	});
	return store_flavour_launch(ctx, true, n_rows, n_rows * ((set || windowed) ? v.length() : ctx->ref_len), launch);
}


int check_batch(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows is NULL");
	if (flags & ~(V2M_SPLICE_UNALIGNED | V2M_SPLICE_BGZF)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
	if (!ctx->has_graph) return fail(ctx, V2M_ERR_STATE, "no graph uploaded");
	if (rows->n_rows && !rows->copy_index && !rows->cut_offsets) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows->copy_index is NULL");
	if (rows->cut_offsets && rows->cut_offsets[rows->n_rows] && (!rows->cut_nodes || !rows->cut_copies))
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "cut arrays are NULL");
	if (rows->n_rows >= 0xFFFFFFFFull) return fail(ctx, V2M_ERR_UNSUPPORTED, "too many rows in one batch");
	// the founder searches' edge-major copy of the path matrix (as large as the matrix) is not kept through the output that follows them
	if (ctx->d_by_edge.p) { ctx->d_by_edge.reset(); ctx->by_edge_valid = false; }
	if ((flags & V2M_SPLICE_UNALIGNED) && ctx->has_nul_byte)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "the reference sequence or an ALT label holds a NUL byte, which the unaligned kernels use as their padding marker; aligned mode keeps such bytes");
	return V2M_OK;
}


// How a row call cuts its batch into slices: row pitch, rows per slice, slice count and the bytes of a slice's rows.  Slices of
// 512 MB; of 128 MB for batches of less than 8 GB (a founder run's 26 rows): a gigabyte of pinned memory takes 0.15 s to set up and as
// long to give back, which a run of a second notices (config 4 end to end: 1.39 -> 1.22 s).  max_rows_per_slice: a limit of the
// caller's (BGZF's member slots); table_bytes_per_row: what a row takes in device tables beside its bytes, counted against the slot
// (the distinct call's keys, lengths, pairs and flags).
struct slice_plan { u64 pitch, rows_per_slice, n_slices, slot_bytes; };

slice_plan plan_slices(v2m_ctx const *ctx, u64 n_rows, bool unaligned, u64 max_rows_per_slice = ~u64(0), u64 table_bytes_per_row = 0)
{
	slice_plan p;
	p.pitch = ctx->set_call ? ctx->set.pitch : unaligned ? ((v2m_max_unaligned_length(ctx) + 255) & ~u64(255)) : v2m_min_row_pitch(ctx);
	char const *const slot_env(std::getenv("V2M_RING_SLOT_BYTES"));   // test knob: force small slices
	u64 const slot_default(n_rows * p.pitch < (u64(8) << 30) ? (u64(128) << 20) : (u64(512) << 20));
	u64 const slot_target((slot_env && *slot_env) ? std::strtoull(slot_env, nullptr, 10) : slot_default);
	p.rows_per_slice = std::max<u64>(1, std::min<u64>({n_rows, slot_target / (p.pitch + table_bytes_per_row), max_rows_per_slice}));
	p.n_slices = (n_rows + p.rows_per_slice - 1) / p.rows_per_slice;
	p.slot_bytes = p.rows_per_slice * p.pitch;
	return p;
}

// The first n of the context's pinned slots, each of at least `bytes`.  No row of theirs may be held (wait_released).
int ensure_host_slots(v2m_ctx *ctx, u64 n, u64 bytes)
{
	while (ctx->host_slots.size() < n) {
		std::unique_ptr<v2m_row_hold> slot(new v2m_row_hold);
		slot->ring = &ctx->held_state;
		V2M_HIP_TRY(ctx, hipEventCreateWithFlags(&slot->copied, hipEventDisableTiming));
		ctx->host_slots.push_back(std::move(slot));
	}
	for (u64 i(0); i < n; ++i) V2M_HIP_TRY(ctx, ctx->host_slots[i]->host.ensure(bytes));
	return V2M_OK;
}

void wait_released(v2m_ctx *ctx, v2m_row_hold &slot)
{
	std::unique_lock<std::mutex> lock(ctx->held_state.mutex);
	ctx->held_state.released.wait(lock, [&] { return 0 == slot.outstanding; });
}


// ---- BGZF (bgzf_kernels.hpp) ------------------------------------------------------------------

u64 bgzf_pieces(u64 n) { return (n + v2m::kBgzfBlockBytes - 1) / v2m::kBgzfBlockBytes; }

// Queues the encoder for n_rows rows at d_rows (row r at d_rows + r * pitch; lengths on the device, or `length` for every row when
// d_lengths is NULL) whose longest row has at most max_len bytes: the members densely into d_dense, and the row extents
// (n_rows + 1 offsets into d_dense, the last one the total) into ctx->d_bgzf_table.  The grid is n_rows x the pieces of max_len;
// the workgroups past a row's end write a member size of 0.
int bgzf_encode_rows(v2m_ctx *ctx, char const *d_rows, u64 pitch, u64 const *d_lengths, u64 length, u64 max_len, u64 n_rows, char *d_dense)
{
	u64 const per_row(std::max<u64>(1, bgzf_pieces(max_len)));
	u64 const n_blocks(n_rows * per_row);
	if (n_blocks > 0x7FFFFFFFull || per_row > 0xFFFFFFFFull)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "BGZF grid too large (%llu blocks); use smaller batches", (unsigned long long) n_blocks);
	V2M_HIP_TRY(ctx, ctx->d_bgzf_slots.ensure(n_blocks * v2m::kBgzfSlotBytes));
	V2M_HIP_TRY(ctx, ctx->d_bgzf_sizes.ensure(n_blocks * sizeof(u32)));
	V2M_HIP_TRY(ctx, ctx->d_bgzf_offsets.ensure(n_blocks * sizeof(u64)));
	V2M_HIP_TRY(ctx, ctx->d_bgzf_table.ensure((n_rows + 1) * sizeof(u64)));
	{
		timed_launch tl(ctx, V2M_KERNEL_BGZF);
		hipLaunchKernelGGL(v2m::bgzf_deflate_kernel, dim3(unsigned(n_blocks)), dim3(v2m::kBgzfThreads), 0, ctx->stream,
			d_rows, pitch, d_lengths, length, u32(per_row), ctx->d_bgzf_slots.as<char>(), ctx->d_bgzf_sizes.as<u32>());
		hipLaunchKernelGGL(v2m::bgzf_scan_kernel, dim3(1), dim3(v2m::kBgzfScanThreads), 0, ctx->stream,
			ctx->d_bgzf_sizes.as<u32>(), n_blocks, u32(per_row), n_rows, ctx->d_bgzf_offsets.as<u64>(), ctx->d_bgzf_table.as<u64>());
		hipLaunchKernelGGL(v2m::bgzf_compact_kernel, dim3(unsigned(n_blocks)), dim3(256), 0, ctx->stream,
			ctx->d_bgzf_slots.as<char>(), ctx->d_bgzf_sizes.as<u32>(), ctx->d_bgzf_offsets.as<u64>(), d_dense);
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}


// v2m_splice_rows with V2M_SPLICE_BGZF.  The slices of v2m_splice_rows with the encoder after every slice's splice: slice s's members
// are compacted into d_bgzf_dense[s & 1] and its row extents come back on the compute stream; the host reads the slice's total only
// after slice s + 1 has been queued and then copies just the compressed bytes into pinned slot s & 1 on the copy stream, so the link
// and the kernels still overlap.  The dense buffers and pinned slots are sized by the worst case (v2m_bgzf_bound per row: tiny rows
// expand), and a slice is cut so that its 64-KiB member slots stay within 1 GiB.
int splice_rows_bgzf(v2m_ctx *ctx, v2m_row_batch const *rows, bool unaligned, v2m_sink_fn sink, void *user)
{
	u64 const L(ctx->view().length());
	u64 const max_len(unaligned ? v2m_max_unaligned_length(ctx) : L);
	u64 const member_slots_per_row(std::max<u64>(1, bgzf_pieces(max_len)) * v2m::kBgzfSlotBytes);
	slice_plan const p(plan_slices(ctx, rows->n_rows, unaligned, (u64(1) << 30) / member_slots_per_row));
	u64 const pitch(p.pitch), rows_per_slice(p.rows_per_slice), n_slices(p.n_slices);
	u64 const dense_bytes(rows_per_slice * v2m_bgzf_bound(max_len));
	int const n_buffers(n_slices > 1 ? 2 : 1);
	for (int i(0); i < n_buffers; ++i) {
		V2M_HIP_TRY(ctx, ctx->ring[i].ensure(p.slot_bytes));
		V2M_HIP_TRY(ctx, ctx->d_bgzf_dense[i].ensure(dense_bytes));
		V2M_HIP_TRY(ctx, ctx->h_bgzf_table[i].ensure((rows_per_slice + 1) * sizeof(u64)));
	}
	if (int const rc = ensure_host_slots(ctx, n_buffers, dense_bytes)) return rc;
	std::vector<u64> extents[2];
	auto const slice_rows([&](u64 s, u64 &r0, u64 &r1) { r0 = s * rows_per_slice; r1 = std::min(rows->n_rows, r0 + rows_per_slice); });

	auto const launch([&](u64 s) -> int {
		int const b(int(s & 1));
		u64 r0, r1;
		slice_rows(s, r0, r1);
		if (s >= 2) V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->host_slots[b]->copied, 0));   // d_bgzf_dense[b] has crossed the link
		V2M_HIP_TRY(ctx, ctx->ring[b].ensure(p.slot_bytes));                 // (the slice takes its device slots: refilled in the checked build)
		V2M_HIP_TRY(ctx, ctx->d_bgzf_dense[b].ensure(dense_bytes));
		if (int const rc = unaligned
				? splice_unaligned_slice(ctx, rows, r0, r1, ctx->ring[b].as<char>(), pitch)
				: splice_aligned_slice(ctx, rows, r0, r1, ctx->ring[b].as<char>(), pitch))
			return rc;
		if (int const rc = bgzf_encode_rows(ctx, ctx->ring[b].as<char>(), pitch, unaligned ? ctx->d_row_lengths.as<u64>() : nullptr, L, max_len, r1 - r0, ctx->d_bgzf_dense[b].as<char>()))
			return rc;
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_bgzf_table[b].p, ctx->d_bgzf_table.p, (r1 - r0 + 1) * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipEventRecord(ctx->ev_compute[b], ctx->stream));
		return V2M_OK;
	});
	auto const issue_copy([&](u64 s) -> int {
		int const b(int(s & 1));
		u64 r0, r1;
		slice_rows(s, r0, r1);
		V2M_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_compute[b]));
		u64 const *const table(ctx->h_bgzf_table[b].as<u64>());
		extents[b].assign(table, table + (r1 - r0 + 1));
		pinned_buf &host(ctx->host_slots[b]->host);
		if (extents[b].back() > host.bytes)
			return fail(ctx, V2M_ERR_HIP, "BGZF members of rows %llu.. exceed their bound", (unsigned long long) r0);
		V2M_POISON_HOST(host.p, extents[b].back());
		if (extents[b].back())
			V2M_HIP_TRY(ctx, hipMemcpyAsync(host.p, ctx->d_bgzf_dense[b].p, extents[b].back(), hipMemcpyDeviceToHost, ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipEventRecord(ctx->host_slots[b]->copied, ctx->copy_stream));
		return V2M_OK;
	});
	auto const drain([&](u64 s) -> int {
		int const b(int(s & 1));
		u64 r0, r1;
		slice_rows(s, r0, r1);
		V2M_HIP_TRY(ctx, hipEventSynchronize(ctx->host_slots[b]->copied));
		char const *const base(ctx->host_slots[b]->host.as<char>());
		for (u64 r(r0); r < r1; ++r) {
			u64 const begin(extents[b][r - r0]), end(extents[b][r - r0 + 1]);
			if (sink(user, r, base + begin, end - begin)) return fail(ctx, V2M_ERR_SINK, "sink aborted at row %llu", (unsigned long long) r);
		}
		return V2M_OK;
	});

	int rc(V2M_OK);
	u64 launched(0), copied(0), drained(0);
	for (u64 s(0); s < n_slices && V2M_OK == rc; ++s) {
		if (V2M_OK != (rc = launch(s))) break;
		launched = s + 1;
		if (s >= 1) { if (V2M_OK != (rc = issue_copy(s - 1))) break; copied = s; }
		if (s >= 2) { if (V2M_OK != (rc = drain(s - 2))) break; drained = s - 1; }
	}
	while (V2M_OK == rc && copied < launched) { rc = issue_copy(copied); if (V2M_OK == rc) ++copied; }
	while (V2M_OK == rc && drained < copied) { rc = drain(drained); if (V2M_OK == rc) ++drained; }
	(void) hipStreamSynchronize(ctx->stream);
	(void) hipStreamSynchronize(ctx->copy_stream);
	return rc;
}


// Rows [r0, r1) of a slice in a pinned slot: row r at base + (r - r0) * pitch, with lengths[r - r0] bytes (unaligned) or `length`.
struct slot_rows {
	u64 r0, r1;
	char const *base;
	u64 pitch, length;
	u64 const *lengths;
	u32 const *set_lengths;   // a window set in unaligned mode: [r1 - r0][n_windows]
	char const *row(u64 r) const { return base + (r - r0) * pitch; }
	u64 bytes(u64 r) const { return lengths ? lengths[r - r0] : length; }
};

// v2m_splice_rows and v2m_splice_rows_held.  Slices of the batch alternate between two device slots and go round the first n_slots
// pinned slots: the D2H copy of slice s runs on copy_stream while the kernels of slice s + 1 run on stream, and then
// deliver(slot, slot_rows) hands slice s to the sink.  A slot is copied into again only when its rows are all released (a deliver
// that holds none leaves nothing to wait for), and when the call returns, both streams are idle and no row is held.  `name` labels
// the V2M_SPLICE_TIMING line.
template <typename F>
int splice_rows_pipeline(v2m_ctx *ctx, v2m_row_batch const *rows, bool unaligned, u64 n_slots, char const *name, F const &deliver)
{
	u64 const L(ctx->view().length());
	if (0 == L) {   // rows without a byte: nothing to copy, nothing to hold on to
		if (int const rc = ensure_host_slots(ctx, 1, 0)) return rc;
		int const rc(deliver(*ctx->host_slots[0], slot_rows{0, rows->n_rows, "", 0, 0, nullptr, nullptr}));
		wait_released(ctx, *ctx->host_slots[0]);
		return rc;
	}
	slice_plan const p(plan_slices(ctx, rows->n_rows, unaligned));
	// unaligned: row lengths ride at the end of the pinned slot (of a window set: the slice's [rows][n_windows] lengths table)
	bool const set_lengths(ctx->set_call && unaligned);
	u64 const lengths_bytes(set_lengths ? ((p.rows_per_slice * ctx->set.n_windows * sizeof(u32) + 7) & ~u64(7)) : p.rows_per_slice * sizeof(u64));
	u64 const slots_used(std::min(n_slots, p.n_slices));
	for (int i(0); i < (p.n_slices > 1 ? 2 : 1); ++i) V2M_HIP_TRY(ctx, ctx->ring[i].ensure(p.slot_bytes));
	if (int const rc = ensure_host_slots(ctx, slots_used, p.slot_bytes + lengths_bytes)) return rc;
	auto const slot_of([&](u64 s) -> v2m_row_hold & { return *ctx->host_slots[s % n_slots]; });
	auto const first_row([&](u64 s) { return s * p.rows_per_slice; });
	auto const end_row([&](u64 s) { return std::min(rows->n_rows, (s + 1) * p.rows_per_slice); });

	auto const issue([&](u64 s) -> int {
		v2m_row_hold &slot(slot_of(s));
		int const d(int(s & 1));
		u64 const r0(first_row(s)), r1(end_row(s));
		wait_released(ctx, slot);                                             // the slice that was here n_slots slices ago
		// the device slot is written again only when the copy that reads it (slice s - 2) is over
		if (s >= 2) V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, slot_of(s - 2).copied, 0));
		V2M_HIP_TRY(ctx, ctx->ring[d].ensure(p.slot_bytes));                 // (the slice takes its device slot: refilled in the checked build)
		V2M_POISON_HOST(slot.host.p, p.slot_bytes + lengths_bytes);
		ctx->set_lengths_slot = d;   // (a window set's lengths table is rewritten, like the device slot, only after slice s - 2's copies)
		if (int const rc = unaligned
				? splice_unaligned_slice(ctx, rows, r0, r1, ctx->ring[d].as<char>(), p.pitch)
				: splice_aligned_slice(ctx, rows, r0, r1, ctx->ring[d].as<char>(), p.pitch))
			return rc;
		if (unaligned && !set_lengths)   // d_row_lengths is reused by the next slice: take the copy on the compute stream
			V2M_HIP_TRY(ctx, hipMemcpyAsync(slot.host.as<char>() + p.slot_bytes, ctx->d_row_lengths.p, (r1 - r0) * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipEventRecord(ctx->ev_compute[d], ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute[d], 0));
		if (set_lengths)   // the lengths table has a buffer per device slot: it travels on the copy stream, ahead of the rows it describes
			V2M_HIP_TRY(ctx, hipMemcpyAsync(slot.host.as<char>() + p.slot_bytes, ctx->d_set_lengths[d].p, (r1 - r0) * ctx->set.n_windows * sizeof(u32), hipMemcpyDeviceToHost, ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(slot.host.p, ctx->ring[d].p, (r1 - r0) * p.pitch, hipMemcpyDeviceToHost, ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipEventRecord(slot.copied, ctx->copy_stream));
		return V2M_OK;
	});
	auto const hand_over([&](u64 s) -> int {
		v2m_row_hold &slot(slot_of(s));
		V2M_HIP_TRY(ctx, hipEventSynchronize(slot.copied));
		char const *const base(slot.host.as<char>());
		return deliver(slot, slot_rows{first_row(s), end_row(s), base, p.pitch, L, (unaligned && !set_lengths) ? reinterpret_cast<u64 const *>(base + p.slot_bytes) : nullptr,
			set_lengths ? reinterpret_cast<u32 const *>(base + p.slot_bytes) : nullptr});
	});

	// V2M_SPLICE_TIMING=1: where the host's time of this call went (row tables + launches / waiting for copies + the sink), to stderr
	bool const timing(nullptr != std::getenv("V2M_SPLICE_TIMING"));
	double t_issue(0), t_drain(0);
	auto const now([] { return std::chrono::steady_clock::now(); });
	auto const since([&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); });
	auto const t_call(now());

	int rc(V2M_OK);
	u64 launched(0);
	for (u64 s(0); s < p.n_slices && V2M_OK == rc; ++s) {
		auto const t_slice(now());
		rc = issue(s);
		t_issue += since(t_slice);
		if (V2M_OK != rc) break;
		launched = s + 1;
		auto const t_d(now());
		if (s >= 1) rc = hand_over(s - 1);                                   // its copy ran under this slice's kernels
		t_drain += since(t_d);
	}
	auto const t_d(now());
	if (V2M_OK == rc && launched) rc = hand_over(launched - 1);
	t_drain += since(t_d);
	// leave both streams idle and every slot released whatever happened (the slots are the library's)
	(void) hipStreamSynchronize(ctx->stream);
	(void) hipStreamSynchronize(ctx->copy_stream);
	for (u64 i(0); i < slots_used; ++i) wait_released(ctx, *ctx->host_slots[i]);
	if (timing) std::fprintf(stderr, "[%s] %llu rows in %llu slices: %.3f s in all, %.3f s preparing and launching, %.3f s waiting for copies and in the sink\n",
		name, (unsigned long long) rows->n_rows, (unsigned long long) p.n_slices, since(t_call), t_issue, t_drain);
	return rc;
}


// CRC-32 (IEEE, reflected 0xEDB88320) of n host bytes.
uint32_t crc32_host(unsigned char const *p, u64 n)
{
	static uint32_t const *const table([] {
		static uint32_t t[256];
		for (uint32_t i(0); i < 256; ++i) {
			uint32_t c(i);
			for (int k(0); k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
			t[i] = c;
		}
		return t;
	}());
	uint32_t c(0xFFFFFFFFu);
	for (u64 i(0); i < n; ++i) c = table[(c ^ p[i]) & 255] ^ (c >> 8);
	return ~c;
}

} // namespace


// =============================================================================================
namespace {

// Calls launch(std::integral_constant<int, kPer>) with the founder kernels' instantiation for `copies` chromosome copies (the larger of the copies
// walked and the bound matrix's columns: a thread owns kPer copies of the order, and the LDS arrays -- the staged edge column among them -- hold
// 1024 * kPer): every count up to 8, then 10, 12, 16 and 20.
template <int kMaxPer, typename t_launch>
void pbwt_dispatch_per_thread(u64 copies, t_launch &&launch)
{
	static_assert(20 == v2m::kPbwtPerThread && 20 == v2m::kPbwtPerThreadRecords && 20 == kMaxPer, "one case per instantiation");
	u64 const per((copies + v2m::kPbwtThreads - 1) / v2m::kPbwtThreads);      // (<= kMaxPer was checked)
	switch (per) {
		case 0: case 1: launch(std::integral_constant<int, 1>{}); return;
		case 2: launch(std::integral_constant<int, 2>{}); return;
		case 3: launch(std::integral_constant<int, 3>{}); return;
		case 4: launch(std::integral_constant<int, 4>{}); return;
		case 5: launch(std::integral_constant<int, 5>{}); return;
		case 6: launch(std::integral_constant<int, 6>{}); return;
		case 7: launch(std::integral_constant<int, 7>{}); return;
		case 8: launch(std::integral_constant<int, 8>{}); return;
		case 9: case 10: launch(std::integral_constant<int, 10>{}); return;
		case 11: case 12: launch(std::integral_constant<int, 12>{}); return;
		default: break;
	}
	if constexpr (kMaxPer > 12) {
		if (per <= 16) launch(std::integral_constant<int, 16>{});
		else launch(std::integral_constant<int, 20>{});
	}
}

} // namespace


// ---- BGZF input (bgzf_kernels.hpp: bgzf_inflate_kernel) ---------------------------------------------
namespace {

char const *inflate_status_text(u32 st)
{
	static char const *const text[v2m::kInflateStatusCount] = {"ok", "invalid block type", "stored block lengths do not match (LEN != ~NLEN)",
		"too many length or distance symbols (HLIT > 286 or HDIST > 30)", "invalid code-length code (over-subscribed, incomplete or undecodable)",
		"invalid code-length repeat (no previous length, or past HLIT + HDIST)", "invalid literal/length code (over-subscribed or incomplete)",
		"invalid distance code (over-subscribed or incomplete)", "no end-of-block code", "invalid literal/length symbol",
		"invalid distance symbol", "distance too far back", "output longer than ISIZE", "the deflate stream reads past the payload",
		"output shorter than ISIZE", "CRC-32 mismatch", "bad framing"};
	return st < v2m::kInflateStatusCount ? text[st] : "unknown status";
}

unsigned char const kBgzfEofMember[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// The members of n bytes of BGZF (the framing of include/v2m_hip.h): offsets[k] = member k's first byte (and offsets[members] = n),
// isize[k] = its ISIZE.  On failure: a V2M_ERR_* code with the message in `what`.
struct bgzf_members {
	std::vector<u64> offsets;
	std::vector<u32> isize;
	u64 bytes{};
	bool ends_with_eof{};
};

int walk_error(std::string &what, int code, char const *fmt, ...)
{
	char buf[320];
	va_list ap;
	va_start(ap, fmt);
	std::vsnprintf(buf, sizeof(buf), fmt, ap);
	va_end(ap);
	what = buf;
	return code;
}

int bgzf_walk(unsigned char const *src, u64 n, bgzf_members &out, std::string &what)
{
	auto const le16([&](u64 i) { return u32(src[i]) | (u32(src[i + 1]) << 8); });
	auto const le32([&](u64 i) { return le16(i) | (le16(i + 2) << 16); });
	u32 const head_bytes(v2m::kBgzfHeaderBytes), foot_bytes(v2m::kBgzfFooterBytes);
	out = bgzf_members{};
	u64 pos(0);
	while (pos < n) {
		unsigned long long const at(pos), left(n - pos);
		if (left < 2 || 0x1f != src[pos] || 0x8b != src[pos + 1])
			return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: no gzip magic (1f 8b)", at);
		bool const bgzf_header(left >= 16 && 8 == src[pos + 2] && 4 == src[pos + 3] && 6 == le16(pos + 10) && 'B' == src[pos + 12] && 'C' == src[pos + 13]
			&& 2 == le16(pos + 14));
		if (!bgzf_header) {
			if (0 == pos && left >= 4 && 8 == src[2] && 0 == (src[3] & 0xe0))   // a gzip header, deflate, valid flags: gzip, but not BGZF
				return walk_error(what, V2M_ERR_UNSUPPORTED, "the input is gzip but not BGZF (its first member has no BC extra subfield); recompress it with bgzip");
			if (left < 16) return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: truncated header (%llu bytes left)", at, left);
			return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: not a BGZF header (1f 8b 08 04, XLEN 6, one BC subfield of SLEN 2)", at);
		}
		if (left < head_bytes) return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: truncated header (%llu bytes left)", at, left);
		unsigned long long const size(le16(pos + 16) + 1ull);
		if (size < head_bytes + foot_bytes)
			return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: BSIZE %llu is shorter than a header and footer", at, size - 1);
		if (size > left)
			return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: BSIZE says %llu bytes, the input ends %llu bytes later (truncated)", at, size, left);
		u32 const isize(le32(pos + size - 4));
		if (isize > v2m::kBgzfSlotBytes)
			return walk_error(what, V2M_ERR_INVALID_ARGUMENT, "BGZF member at compressed offset %llu: ISIZE %llu is above 65536", at, (unsigned long long) isize);
		out.offsets.push_back(pos);
		out.isize.push_back(isize);
		out.bytes += isize;
		out.ends_with_eof = sizeof(kBgzfEofMember) == size && 0 == std::memcmp(src + pos, kBgzfEofMember, size);
		pos += size;
	}
	out.offsets.push_back(n);
	return V2M_OK;
}

// memcpy on up to 8 threads for large copies (pageable <-> pinned).
void host_copy(void *dst, void const *src, u64 n)
{
	u64 const piece(u64(8) << 20);
	unsigned const k(unsigned(std::min<u64>(8, n / piece)));
	if (k < 2) { std::memcpy(dst, src, n); return; }
	u64 const share((n / k + 4095) & ~u64(4095));
	std::vector<std::thread> pool;
	for (unsigned t(1); t < k; ++t) {
		u64 const a(std::min(n, t * share)), b(std::min(n, a + share));
		if (a < b) pool.emplace_back([=] { std::memcpy(static_cast<char *>(dst) + a, static_cast<char const *>(src) + a, b - a); });
	}
	std::memcpy(dst, src, std::min(n, share));
	for (auto &th : pool) th.join();
}

} // namespace


extern "C" {

uint32_t v2m_abi_version(void) { return V2M_ABI_VERSION; }

int v2m_ctx_create(int device_id, v2m_ctx **ctx_out)
{
	if (!ctx_out) return fail(nullptr, V2M_ERR_INVALID_ARGUMENT, "ctx_out is NULL");
	*ctx_out = nullptr;
	int count(0);
	hipError_t st(hipGetDeviceCount(&count));
	if (hipSuccess != st || 0 == count)
		return fail(nullptr, V2M_ERR_NO_DEVICE, "no HIP device available (%s); this library has no CPU fallback", hipSuccess != st ? hipGetErrorString(st) : "device count is 0");
	if (device_id < 0 || device_id >= count)
		return fail(nullptr, V2M_ERR_INVALID_ARGUMENT, "device %d out of range (%d devices)", device_id, count);
	hipDeviceProp_t prop;
	st = hipGetDeviceProperties(&prop, device_id);
	if (hipSuccess != st) return fail(nullptr, V2M_ERR_HIP, "hipGetDeviceProperties: %s", hipGetErrorString(st));
	if (0 != std::strncmp(prop.gcnArchName, "gfx950", 6))
		return fail(nullptr, V2M_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
	st = hipSetDevice(device_id);
	if (hipSuccess != st) return fail(nullptr, V2M_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(st));
#ifdef V2M_CHECKED_BUILD
	{   // the poison of this context's LDS and scratch (kernels.hpp): V2M_POISON_SEED, decimal or 0x-hex
		char const *const e(std::getenv("V2M_POISON_SEED"));
		u32 const seed((e && *e) ? u32(std::strtoul(e, nullptr, 0)) : 0x9E3779B9u);
		g_poison_seed = seed;
		st = hipMemcpyToSymbol(HIP_SYMBOL(v2m_lds_poison_seed), &seed, sizeof(seed));
		if (hipSuccess != st) return fail(nullptr, V2M_ERR_HIP, "hipMemcpyToSymbol(v2m_lds_poison_seed): %s", hipGetErrorString(st));
	}
#endif

	auto *ctx(new v2m_ctx);
	ctx->device = device_id;
	if (prop.multiProcessorCount > 0) ctx->n_cus = u32(prop.multiProcessorCount);
	if (hipSuccess != (st = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking))
		|| hipSuccess != (st = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking))) {
		delete ctx;
		return fail(nullptr, V2M_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(st));
	}
	for (int i(0); i < 2 && hipSuccess == st; ++i) {
		st = hipEventCreateWithFlags(&ctx->ev_compute[i], hipEventDisableTiming);
		if (hipSuccess == st) st = hipEventCreateWithFlags(&ctx->ev_row_stage[i], hipEventDisableTiming);
		if (hipSuccess == st) st = hipEventCreateWithFlags(&ctx->ev_inflate_in[i], hipEventDisableTiming);
	}
	if (hipSuccess != st) {
		std::string const what(hipGetErrorString(st));
		v2m_ctx_destroy(ctx);   // destroys whatever was created
		return fail(nullptr, V2M_ERR_HIP, "hipEventCreateWithFlags: %s", what.c_str());
	}
#ifdef V2M_CHECKED_BUILD
	char seed_info[64];
	std::snprintf(seed_info, sizeof(seed_info), "checked build: poison seed 0x%08x", g_poison_seed.load());
	ctx->info = seed_info;
#endif
	*ctx_out = ctx;
	return V2M_OK;
}

void v2m_ctx_destroy(v2m_ctx *ctx)
{
	if (!ctx) return;
	(void) hipSetDevice(ctx->device);
	(void) hipStreamSynchronize(ctx->stream);
	(void) hipStreamSynchronize(ctx->copy_stream);
	for (auto &v : ctx->events) for (auto &e : v) { (void) hipEventDestroy(e.begin); (void) hipEventDestroy(e.end); }
	for (auto &e : ctx->free_events) { (void) hipEventDestroy(e.begin); (void) hipEventDestroy(e.end); }
	for (int i(0); i < 2; ++i) {
		if (ctx->ev_compute[i]) (void) hipEventDestroy(ctx->ev_compute[i]);
		if (ctx->ev_row_stage[i]) (void) hipEventDestroy(ctx->ev_row_stage[i]);
		if (ctx->ev_inflate_in[i]) (void) hipEventDestroy(ctx->ev_inflate_in[i]);
	}
	for (auto &slot : ctx->host_slots) if (slot && slot->copied) (void) hipEventDestroy(slot->copied);
	(void) hipStreamDestroy(ctx->stream);
	(void) hipStreamDestroy(ctx->copy_stream);
	delete ctx;
}

const char *v2m_last_error(const v2m_ctx *ctx)
{
	return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int v2m_ctx_synchronize(v2m_ctx *ctx)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_stream));
	return V2M_OK;
}

void *v2m_ctx_stream(v2m_ctx *ctx) { return ctx ? (void *) ctx->stream : nullptr; }

const char *v2m_ctx_info(const v2m_ctx *ctx) { return ctx ? ctx->info.c_str() : ""; }


// ---- transpose ------------------------------------------------------------------------------

int v2m_transpose_bits_device(v2m_ctx *ctx, const void *d_src_words, uint64_t n_rows, uint64_t n_cols, void *d_dst_words)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (0 == n_cols) return V2M_OK;                          // transpose_matrix.cc:48-49
	if (n_rows % 64 || n_cols % 64)                          // transpose_matrix.cc:53-54
		return fail(ctx, V2M_ERR_PRECONDITION, "matrix dimensions must be multiples of 64 (got %llu x %llu)", (unsigned long long) n_rows, (unsigned long long) n_cols);
	if (0 == n_rows) return V2M_OK;
	if (!d_src_words || !d_dst_words) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL matrix pointer");
	if (((uintptr_t) d_src_words | (uintptr_t) d_dst_words) & 7) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "matrix pointers must be 8-byte aligned");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	return launch_transpose(ctx, static_cast<u64 const *>(d_src_words), n_rows, n_cols, static_cast<u64 *>(d_dst_words));
}

int v2m_transpose_bits(v2m_ctx *ctx, const uint64_t *src_words, uint64_t n_rows, uint64_t n_cols, uint64_t *dst_words)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (0 == n_cols) return V2M_OK;
	if (n_rows % 64 || n_cols % 64)
		return fail(ctx, V2M_ERR_PRECONDITION, "matrix dimensions must be multiples of 64 (got %llu x %llu)", (unsigned long long) n_rows, (unsigned long long) n_cols);
	if (0 == n_rows) return V2M_OK;
	if (!src_words || !dst_words) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL matrix pointer");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	size_t const bytes(n_rows / 64 * n_cols * sizeof(u64));
	dev_buf src, dst;
	V2M_HIP_TRY(ctx, src.ensure(bytes));
	V2M_HIP_TRY(ctx, dst.ensure(bytes));
	V2M_HIP_TRY(ctx, hipMemcpyAsync(src.p, src_words, bytes, hipMemcpyHostToDevice, ctx->stream));
	if (int const rc = launch_transpose(ctx, src.as<u64>(), n_rows, n_cols, dst.as<u64>())) return rc;
	V2M_HIP_TRY(ctx, hipMemcpyAsync(dst_words, dst.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return V2M_OK;
}


// ---- graph ----------------------------------------------------------------------------------

int v2m_upload_graph(v2m_ctx *ctx, const v2m_graph_view *g, const char *ref_seq, uint64_t ref_len)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!g) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "graph is NULL");
	u64 const N(g->node_count), E(g->edge_count);
	if (0 == N) return fail(ctx, V2M_ERR_PRECONDITION, "a variant graph has at least the source node");
	if (!g->reference_positions || !g->aligned_positions || !g->alt_edge_count_csum) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL node array");
	if (E && (!g->alt_edge_targets || !g->alt_edge_label_offsets)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL edge array");
	if (ref_len && !ref_seq) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "ref_seq is NULL");
	if (g->paths_by_chrom_copy_and_edge && (g->path_rows % 64 || g->path_cols % 64 || g->path_rows < E))
		return fail(ctx, V2M_ERR_PRECONDITION, "path matrix must be (>= edge_count) x copies with both dimensions multiples of 64");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	u64 const limit32(0xFFFFFFFFull - 2 * v2m::kTileBytes);
	u64 const L(g->aligned_positions[N - 1]);
	if (N >= limit32 || E >= limit32 || L >= limit32 || ref_len >= limit32)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "graph does not fit 32-bit device indices (nodes %llu, edges %llu, aligned length %llu)", (unsigned long long) N, (unsigned long long) E, (unsigned long long) L);

	// --- validate what output_sequence() silently relies on, narrow to 32 bits -------------
	std::vector<u32> ref_pos(N), aln_pos(N), csum(N + 1);
	if (0 != g->reference_positions[0] || 0 != g->aligned_positions[0])
		return fail(ctx, V2M_ERR_PRECONDITION, "node 0 must be at reference and aligned position 0");
	for (u64 n(0); n < N; ++n) {
		u64 const r(g->reference_positions[n]), a(g->aligned_positions[n]);
		if (r > ref_len) return fail(ctx, V2M_ERR_PRECONDITION, "node %llu: reference position %llu is past the reference (%llu)", (unsigned long long) n, (unsigned long long) r, (unsigned long long) ref_len);
		if (n) {
			u64 const pr(g->reference_positions[n - 1]), pa(g->aligned_positions[n - 1]);
			if (r <= pr) return fail(ctx, V2M_ERR_PRECONDITION, "reference positions must increase strictly (node %llu)", (unsigned long long) n);
			if (a < pa || a - pa < r - pr)   // the '-' count at sequence_writer.cc:81 would underflow
				return fail(ctx, V2M_ERR_PRECONDITION, "node %llu: aligned distance is shorter than the reference distance", (unsigned long long) n);
		}
		ref_pos[n] = u32(r);
		aln_pos[n] = u32(a);
	}
	if (0 != g->alt_edge_count_csum[0] || E != g->alt_edge_count_csum[N])
		return fail(ctx, V2M_ERR_PRECONDITION, "alt_edge_count_csum must run from 0 to edge_count");
	for (u64 n(0); n <= N; ++n) {
		if (n && g->alt_edge_count_csum[n] < g->alt_edge_count_csum[n - 1]) return fail(ctx, V2M_ERR_PRECONDITION, "alt_edge_count_csum decreases at node %llu", (unsigned long long) n);
		csum[n] = u32(g->alt_edge_count_csum[n]);
	}
	if (N >= 1 && csum[N] != csum[N - 1])
		return fail(ctx, V2M_ERR_PRECONDITION, "the sink node cannot have ALT edges");

	std::vector<v2m::edge_span> spans(E);
	std::vector<v2m::edge_patch> patches(E);
	std::vector<u32> tgt_prefix_max(E + 1, 0);
	std::vector<u64> overlappable((E + 63) / 64, 0);   // edge e can be skipped by some row iff src[e] < max tgt[0..e)
	u64 label_total(0);
	if (E) {
		label_total = g->alt_edge_label_offsets[E];
		if (label_total >= limit32) return fail(ctx, V2M_ERR_UNSUPPORTED, "label pool too large");
		if (label_total && !g->alt_edge_label_bytes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "alt_edge_label_bytes is NULL");
		if (0 != g->alt_edge_label_offsets[0]) return fail(ctx, V2M_ERR_PRECONDITION, "alt_edge_label_offsets must start at 0");
	}
	for (u64 n(0); n < N; ++n) {
		for (u32 e(csum[n]); e < csum[n + 1]; ++e) {
			u64 const tgt(g->alt_edge_targets[e]);
			if (tgt <= n || tgt >= N) return fail(ctx, V2M_ERR_PRECONDITION, "edge %u: target %llu must lie after its source node %llu", e, (unsigned long long) tgt, (unsigned long long) n);
			u64 const lo(g->alt_edge_label_offsets[e]), hi(g->alt_edge_label_offsets[e + 1]);
			if (hi < lo || hi > label_total) return fail(ctx, V2M_ERR_PRECONDITION, "edge %u: bad label offsets", e);
			if (hi - lo > u64(aln_pos[tgt]) - aln_pos[n])   // libbio_assert_lte at sequence_writer.cc:61
				return fail(ctx, V2M_ERR_PRECONDITION, "edge %u: label (%llu) is longer than the aligned span (%u)", e, (unsigned long long) (hi - lo), aln_pos[tgt] - aln_pos[n]);
			spans[e] = {u32(n), u32(tgt)};
			patches[e] = {aln_pos[n], aln_pos[tgt], u32(lo), u32(hi - lo)};
			tgt_prefix_max[e + 1] = std::max(tgt_prefix_max[e], u32(tgt));
			if (n < tgt_prefix_max[e]) overlappable[e >> 6] |= u64(1) << (e & 63);
		}
	}

	// --- who can block an overlappable edge ----------------------------------------------------
	// Edge e is skipped only if an EFFECTIVE earlier edge e' ends past e's source node (tgt[e'] > src[e]); if none of those
	// edges is even set in a row, e is effective there without replaying the walk.  Per overlappable edge: the mask of such
	// edges inside e's own 64-edge word (all ones when one lies in an earlier word: the kernel then replays), indexed by
	// the edge's rank among the overlappable ones.
	std::vector<u32> ovl_rank(overlappable.size() + 1, 0);
	std::vector<u64> blocker_masks;
	for (u64 wi(0); wi < overlappable.size(); ++wi) {
		ovl_rank[wi] = u32(blocker_masks.size());
		for (u64 m(overlappable[wi]); m; m &= m - 1) {
			u64 const b(u64(__builtin_ctzll(m))), e(wi * 64 + b);
			u64 mask(0);
			if (tgt_prefix_max[wi * 64] > spans[e].src) mask = ~u64(0);
			else for (u64 k(0); k < b; ++k) if (spans[wi * 64 + k].tgt > spans[e].src) mask |= u64(1) << k;
			blocker_masks.push_back(mask);
		}
	}
	ovl_rank.back() = u32(blocker_masks.size());

	// --- per-tile edge tables ----------------------------------------------------------------
	u32 const n_tiles(u32(std::max<u64>(1, (L + v2m::kTileBytes - 1) / v2m::kTileBytes)));
	std::vector<u32> tile_edge_begin(n_tiles + 1), cross_offsets(n_tiles + 1, 0), cross_edges;
	{
		u32 e(0);
		for (u32 t(0); t <= n_tiles; ++t) {
			u64 const base(u64(t) * v2m::kTileBytes);
			while (e < E && patches[e].aln_begin < base) ++e;
			tile_edge_begin[t] = e;
		}
		tile_edge_begin[n_tiles] = u32(E);
		// an edge crosses into tile t when aln_begin < t*T < aln_end
		std::vector<u32> counts(n_tiles + 1, 0);
		auto for_each_crossing = [&](auto &&fn) {
			for (u32 e2(0); e2 < E; ++e2) {
				u64 const first(u64(patches[e2].aln_begin) / v2m::kTileBytes + 1);
				if (0 == patches[e2].aln_end) continue;
				u64 const last((u64(patches[e2].aln_end) - 1) / v2m::kTileBytes);
				for (u64 t(first); t <= last && t < n_tiles; ++t) fn(u32(t), e2);
			}
		};
		for_each_crossing([&](u32 t, u32) { ++counts[t]; });
		for (u32 t(0); t < n_tiles; ++t) cross_offsets[t + 1] = cross_offsets[t] + counts[t];
		cross_edges.resize(cross_offsets[n_tiles]);
		std::vector<u32> cursor(cross_offsets.begin(), cross_offsets.end() - 1);
		for_each_crossing([&](u32 t, u32 e2) { cross_edges[cursor[t]++] = e2; });
	}

	// --- upload ------------------------------------------------------------------------------
	ctx->has_graph = false;
	ctx->windowed = false;              // a new graph: whole rows again
	ctx->has_set = false;               // ... and no window set
	ctx->n_nodes = N; ctx->n_edges = E; ctx->ref_len = ref_len; ctx->aligned_len = L; ctx->label_bytes = label_total;
	V2M_HIP_TRY(ctx, ctx->d_ref.ensure(std::max<u64>(ref_len, 16)));
	if (ref_len) V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ref.p, ref_seq, ref_len, hipMemcpyHostToDevice, ctx->stream));
	V2M_HIP_TRY(ctx, ctx->d_labels.ensure(std::max<u64>(label_total, 16)));
	if (label_total) V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_labels.p, g->alt_edge_label_bytes, label_total, hipMemcpyHostToDevice, ctx->stream));
	if (int const rc = upload_vec(ctx, ctx->d_ref_pos, ref_pos)) return rc;
	if (int const rc = upload_vec(ctx, ctx->d_aln_pos, aln_pos)) return rc;
	if (int const rc = upload_vec(ctx, ctx->d_spans, spans)) return rc;
	if (int const rc = upload_vec(ctx, ctx->d_patches, patches)) return rc;
	if (int const rc = upload_vec(ctx, ctx->d_overlappable, overlappable)) return rc;
	if (int const rc = upload_vec(ctx, ctx->d_ovl_rank, ovl_rank)) return rc;
	if (int const rc = upload_vec(ctx, ctx->d_blocker_masks, blocker_masks)) return rc;

	// whole rows: every edge word resolved, rows of the effective-edge scratch the edge count in 64-bit words rounded up to a whole
	// 128-B line so that every row starts line-aligned
	row_view &v(ctx->whole);
	v.begin = 0;
	v.end = L;
	v.max_unaligned = ref_len + label_total;
	v.n_tiles = n_tiles;
	v.has_template0 = false;
	ctx->has_ops_ref_before = false;
	v.words = {0, 0, (E + 63) / 64, (((E + 63) / 64) + 15) & ~u64(15)};
	if (int const rc = upload_vec(ctx, v.d_edge_begin, tile_edge_begin)) return rc;
	if (int const rc = upload_vec(ctx, v.d_cross_offsets, cross_offsets)) return rc;
	if (int const rc = upload_vec(ctx, v.d_cross_edges, cross_edges)) return rc;
	if (int const rc = expand_reference(ctx, v, v.d_template, '-')) return rc;

	ctx->d_paths = nullptr;
	ctx->by_edge_valid = false;
	ctx->path_rows = ctx->path_cols = ctx->path_pitch = 0;
	if (g->paths_by_chrom_copy_and_edge) {
		size_t const bytes(g->path_rows / 64 * g->path_cols * sizeof(u64));
		V2M_HIP_TRY(ctx, ctx->owned_paths.ensure(std::max<size_t>(bytes, 16)));
		if (bytes) V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->owned_paths.p, g->paths_by_chrom_copy_and_edge, bytes, hipMemcpyHostToDevice, ctx->stream));
		ctx->d_paths = ctx->owned_paths.as<u64>();
		ctx->path_rows = g->path_rows;
		ctx->path_cols = g->path_cols;
		ctx->path_pitch = g->path_rows / 64;
	}
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

	// The reference streams whatever bytes the FASTA / VCF held (sequence_writer.cc:73-74).  Aligned mode does the same here; the
	// unaligned kernels mark padding with byte 0, so a graph that holds one is refused there (check_batch) instead of losing it.
	ctx->has_nul_byte = (ref_len && std::memchr(ref_seq, 0, ref_len)) || (label_total && std::memchr(g->alt_edge_label_bytes, 0, label_total));
	ctx->h_csum = std::move(csum);
	ctx->h_tgt_prefix_max = std::move(tgt_prefix_max);
	ctx->h_aln_pos = std::move(aln_pos);
	ctx->h_patches = std::move(patches);
	ctx->h_overlappable = std::move(overlappable);
	ctx->h_tile_edge_begin = std::move(tile_edge_begin);
	ctx->h_cross_offsets = std::move(cross_offsets);
	ctx->h_cross_edges = std::move(cross_edges);
	ctx->has_graph = true;
	return V2M_OK;
}

int v2m_set_paths_device(v2m_ctx *ctx, const void *d_words, uint64_t path_rows, uint64_t path_cols)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph) return fail(ctx, V2M_ERR_STATE, "no graph uploaded");
	if (path_rows % 64 || path_cols % 64 || path_rows < ctx->n_edges)
		return fail(ctx, V2M_ERR_PRECONDITION, "path matrix must be (>= edge_count) x copies with both dimensions multiples of 64");
	if (path_rows && path_cols && (!d_words || ((uintptr_t) d_words & 7))) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_words must be a non-NULL 8-byte aligned device pointer");
	ctx->d_paths = static_cast<u64 const *>(d_words);
	ctx->by_edge_valid = false;
	ctx->path_rows = path_rows;
	ctx->path_cols = path_cols;
	ctx->path_pitch = path_rows / 64;
	return V2M_OK;
}

namespace {

// The library's own copy of paths_by_chrom_copy_and_edge keeps every copy's column on a 128-byte line: the column pitch is
// the word count rounded up to 16.  Nobody but the kernels of this file reads that buffer, and with line-aligned
// destination columns the transpose stores whole lines.
u64 aligned_pitch(u64 words) { return (words + 15) & ~u64(15); }

// Transposes a device-resident transpose input (n_rows copies x n_cols edges, column pitch src_pitch words) into the
// ctx-owned, line-aligned path matrix and binds it.  Asynchronous on the ctx's stream.
int transpose_into_owned_paths(v2m_ctx *ctx, u64 const *d_src, u64 n_rows, u64 n_cols, u64 src_pitch)
{
	u64 const pitch(aligned_pitch(n_cols / 64));
	V2M_HIP_TRY(ctx, ctx->owned_paths.ensure(pitch * n_rows * sizeof(u64)));
	// (the pad words between a column's n_cols / 64 words and its pitch are neither written here nor read by any kernel)
	if (int const rc = launch_transpose(ctx, d_src, n_rows, n_cols, ctx->owned_paths.as<u64>(), src_pitch, pitch)) return rc;
	ctx->d_paths = ctx->owned_paths.as<u64>();
	ctx->by_edge_valid = false;
	ctx->path_rows = n_cols;
	ctx->path_cols = n_rows;
	ctx->path_pitch = pitch;
	return V2M_OK;
}

} // namespace

int v2m_bind_path_matrix_device(v2m_ctx *ctx, const void *d_paths_by_edge_and_chrom_copy, uint64_t n_rows, uint64_t n_cols)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph) return fail(ctx, V2M_ERR_STATE, "no graph uploaded");
	if (n_rows % 64 || n_cols % 64)                            // transpose_matrix.cc:53-54
		return fail(ctx, V2M_ERR_PRECONDITION, "matrix dimensions must be multiples of 64 (got %llu x %llu)", (unsigned long long) n_rows, (unsigned long long) n_cols);
	if (n_cols < ctx->n_edges) return fail(ctx, V2M_ERR_PRECONDITION, "path matrix has %llu edge columns, the graph %llu edges", (unsigned long long) n_cols, (unsigned long long) ctx->n_edges);
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	ctx->d_paths = nullptr;
	ctx->by_edge_valid = false;
	ctx->path_rows = ctx->path_cols = ctx->path_pitch = 0;
	if (0 == n_rows || 0 == n_cols) return V2M_OK;
	if (!d_paths_by_edge_and_chrom_copy || ((uintptr_t) d_paths_by_edge_and_chrom_copy & 7)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "the matrix must be a non-NULL 8-byte aligned device pointer");
	return transpose_into_owned_paths(ctx, static_cast<u64 const *>(d_paths_by_edge_and_chrom_copy), n_rows, n_cols, 0);
}

int v2m_upload_path_slice(v2m_ctx *ctx, const uint64_t *src_words, uint64_t n_rows, uint64_t n_cols, uint64_t first_copy, uint64_t n_copies)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (first_copy > n_rows || n_copies > n_rows - first_copy) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "copies [%llu, %llu) are outside the matrix (%llu rows)", (unsigned long long) first_copy, (unsigned long long) (first_copy + n_copies), (unsigned long long) n_rows);
	// one block: the contiguous slice
	u64 const block((n_copies + 7) & ~u64(7));
	return v2m_upload_path_blocks(ctx, src_words, n_rows, n_cols, first_copy, std::max<u64>(block, 8), std::max<u64>(block, 8), first_copy + n_copies);
}

int v2m_upload_path_blocks(v2m_ctx *ctx, const uint64_t *src_words, uint64_t n_rows, uint64_t n_cols, uint64_t first_copy, uint64_t block_copies, uint64_t stride_copies, uint64_t copy_end)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph) return fail(ctx, V2M_ERR_STATE, "no graph uploaded");
	if (n_rows % 64 || n_cols % 64)                            // transpose_matrix.cc:53-54
		return fail(ctx, V2M_ERR_PRECONDITION, "matrix dimensions must be multiples of 64 (got %llu x %llu)", (unsigned long long) n_rows, (unsigned long long) n_cols);
	if (n_cols < ctx->n_edges) return fail(ctx, V2M_ERR_PRECONDITION, "path matrix has %llu edge columns, the graph %llu edges", (unsigned long long) n_cols, (unsigned long long) ctx->n_edges);
	if (first_copy % 8 || block_copies % 8 || stride_copies % 8 || 0 == block_copies || stride_copies < block_copies)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "first_copy, block_copies and stride_copies must be multiples of 8 (whole bytes of the bit-packed columns), 0 < block_copies <= stride_copies");
	if (copy_end > n_rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "copies up to %llu are outside the matrix (%llu rows)", (unsigned long long) copy_end, (unsigned long long) n_rows);
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	ctx->d_paths = nullptr;
	ctx->by_edge_valid = false;
	ctx->path_rows = ctx->path_cols = ctx->path_pitch = 0;

	// this GPU's copies: blocks j = 0, 1, ... at first_copy + j * stride_copies, the last one possibly cut short by copy_end
	u64 n_copies(0), n_blocks(0);
	for (u64 c(first_copy); c < copy_end; c += stride_copies, ++n_blocks) n_copies += std::min(block_copies, copy_end - c);
	if (0 == n_copies || 0 == n_cols) return V2M_OK;              // nothing to bind: rows of this ctx can only be REF rows
	if (!src_words) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL matrix pointer");

	u64 const hp((n_copies + 63) / 64 * 64);                      // the share's row count: this GPU's copies, padded
	size_t const take((n_copies + 7) / 8), src_col_bytes(n_rows / 8), block_bytes(block_copies / 8), stride_bytes(stride_copies / 8);
	bool const whole(take == src_col_bytes && 1 == n_blocks);
	// a packed share gets line-aligned columns too (pitch rounded up to 16 words); the whole matrix is sent as it is
	u64 const src_pitch(whole ? hp / 64 : aligned_pitch(hp / 64));
	size_t const col_bytes(src_pitch * 8), bytes(col_bytes * n_cols);
	V2M_HIP_TRY(ctx, ctx->d_slice_src.ensure(bytes));
	char const *const src(reinterpret_cast<char const *>(src_words) + first_copy / 8);
	if (whole) {
		// the whole matrix: one contiguous copy
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_slice_src.p, src_words, bytes, hipMemcpyHostToDevice, ctx->stream));
	} else {
		// bytes [first_copy / 8 + j * stride_bytes, + block_bytes) of every column, packed block after block into pinned slots by a few
		// host threads and sent slot by slot
		unsigned char const tail_mask((n_copies % 8) ? (unsigned char) ((1u << (n_copies % 8)) - 1) : (unsigned char) 0xFF);
		size_t const slot_cols(std::max<size_t>(1, std::min<size_t>(n_cols, (size_t(64) << 20) / col_bytes)));
		if (int const rc = ensure_host_slots(ctx, 2, slot_cols * col_bytes)) return rc;
		scoped_events sent;
		V2M_HIP_TRY(ctx, sent.create(2));
		size_t slot_index(0);
		for (size_t c0(0); c0 < n_cols; c0 += slot_cols, ++slot_index) {
			size_t const nc(std::min(slot_cols, size_t(n_cols) - c0));
			int const b(int(slot_index & 1));
			if (slot_index >= 2) V2M_HIP_TRY(ctx, hipEventSynchronize(sent[b]));   // the slot's previous upload has left the host buffer
			char *const stage(ctx->host_slots[b]->host.as<char>());
			V2M_POISON_HOST(stage, nc * col_bytes);
			auto const pack([&](size_t lo, size_t hi) {
				for (size_t c(lo); c < hi; ++c) {
					char *const d(stage + c * col_bytes);
					char const *const column(src + (c0 + c) * src_col_bytes);
					size_t done(0);
					for (u64 j(0); j < n_blocks; ++j) {
						size_t const n(std::min(block_bytes, take - done));
						std::memcpy(d + done, column + j * stride_bytes, n);
						done += n;
					}
					d[take - 1] = char((unsigned char) d[take - 1] & tail_mask);   // bits of copies past the share are another GPU's
					if (take < col_bytes) std::memset(d + take, 0, col_bytes - take);
				}
			});
			unsigned const n_threads(unsigned(std::max<size_t>(1, std::min<size_t>(8, nc * col_bytes >> 22))));
			if (n_threads <= 1) pack(0, nc);
			else {
				std::vector<std::thread> pool;
				for (unsigned t(0); t < n_threads; ++t) pool.emplace_back(pack, nc * t / n_threads, nc * (t + 1) / n_threads);
				for (auto &t : pool) t.join();
			}
			V2M_HIP_TRY(ctx, hipMemcpyAsync(static_cast<char *>(ctx->d_slice_src.p) + c0 * col_bytes, stage, nc * col_bytes, hipMemcpyHostToDevice, ctx->stream));
			V2M_HIP_TRY(ctx, hipEventRecord(sent[b], ctx->stream));
		}
	}
	if (int const rc = transpose_into_owned_paths(ctx, ctx->d_slice_src.as<u64>(), hp, n_cols, src_pitch)) return rc;
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->d_slice_src.reset();
	return V2M_OK;
}

uint64_t v2m_aligned_length(const v2m_ctx *ctx) { return (ctx && ctx->has_graph) ? ctx->aligned_len : 0; }
uint64_t v2m_min_row_pitch(const v2m_ctx *ctx) { return (ctx && ctx->has_graph) ? ((ctx->view().length() + 255) & ~u64(255)) : 0; }
uint64_t v2m_max_unaligned_length(const v2m_ctx *ctx) { return (ctx && ctx->has_graph) ? ctx->view().max_unaligned : 0; }
uint64_t v2m_window_length(const v2m_ctx *ctx) { return (ctx && ctx->has_graph) ? ctx->view().length() : 0; }

namespace {

// The per-tile tables of column windows (v2m_set_column_window: one window; v2m_set_window_set: the windows' tiles one after another).
struct window_tile_tables {
	std::vector<u32> edge_begin, edge_end, cross_offsets{0}, cross_edges;
	u32 n_tiles() const { return u32(edge_end.size()); }   // (edge_begin may carry one more entry: the [n_tiles + 1] shape of tile_tables)
};

u32 first_edge_beginning_at(v2m_ctx const *ctx, u64 col)   // first edge with aln_begin >= col
{
	auto const &patches(ctx->h_patches);
	return u32(std::partition_point(patches.begin(), patches.end(), [&](v2m::edge_patch const &p) { return p.aln_begin < col; }) - patches.begin());
}

// Appends the tiles of the window [col_begin, col_end).  Tile t of the window is columns [B_t, B_t + kTileBytes) clipped to col_end,
// B_t = col_begin + t * kTileBytes.  Its range: the edges that begin in it (edges are ordered by aligned begin).  Its crossing edges
// (aln_begin < B_t < aln_end): those of the whole-row tile T = B_t / kTileBytes that still reach past B_t, then those that begin in
// [T * kTileBytes, B_t) and reach past it -- ascending.
void append_window_tiles(v2m_ctx const *ctx, u64 col_begin, u64 col_end, window_tile_tables &tb)
{
	auto const &patches(ctx->h_patches);
	u64 const n_tiles((col_end - col_begin + v2m::kTileBytes - 1) / v2m::kTileBytes);
	u32 begin(first_edge_beginning_at(ctx, col_begin));
	for (u64 t(0); t < n_tiles; ++t) {
		u64 const B(col_begin + t * v2m::kTileBytes), T(B / v2m::kTileBytes);
		u32 const end(first_edge_beginning_at(ctx, std::min<u64>(B + v2m::kTileBytes, col_end)));
		for (u32 i(ctx->h_cross_offsets[T]); i < ctx->h_cross_offsets[T + 1]; ++i)
			if (patches[ctx->h_cross_edges[i]].aln_end > B) tb.cross_edges.push_back(ctx->h_cross_edges[i]);
		for (u32 e(ctx->h_tile_edge_begin[T]); e < begin; ++e)
			if (patches[e].aln_end > B) tb.cross_edges.push_back(e);
		tb.edge_begin.push_back(begin);
		tb.edge_end.push_back(end);
		tb.cross_offsets.push_back(u32(tb.cross_edges.size()));
		begin = end;
	}
}

// The edges a window's rows depend on, [e_lo, e_hi): from the first edge whose span reaches past col_begin (the running maximum of the
// edges' targets is ordered, and so are the targets' aligned positions) to the last one that begins before col_end (e_hi: the end of
// the window's last tile's range).  Empty when no edge reaches into the window.
u64 first_edge_reaching_past(v2m_ctx const *ctx, u64 col_begin, u32 e_hi)
{
	u64 e_lo(0), hi(e_hi);
	while (e_lo < hi) {
		u64 const mid((e_lo + hi) / 2);
		if (ctx->h_aln_pos[ctx->h_tgt_prefix_max[mid + 1]] > col_begin) hi = mid; else e_lo = mid + 1;
	}
	return e_lo;
}

// The edge words resolve decides for edges [e_lo, e_hi) (none when the range is empty).  Their restart points (the nearest earlier edge
// that is not overlappable, kernels.hpp) lie at or after the last word whose first edge is not overlappable.
word_range words_of_edges(v2m_ctx const *ctx, u64 e_lo, u64 e_hi)
{
	u64 restart(0), lo(0), word_hi(0);   // no edge reaches into the columns: nothing to resolve
	if (e_lo < e_hi) {
		lo = e_lo / 64;
		word_hi = (e_hi + 63) / 64;
		restart = lo;
		while (restart > 0 && (ctx->h_overlappable[restart] & 1)) --restart;
	}
	return {restart, lo, word_hi, (word_hi - restart + 15) & ~u64(15)};
}

} // namespace


int v2m_set_column_window(v2m_ctx *ctx, uint64_t col_begin, uint64_t col_end)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph) return fail(ctx, V2M_ERR_STATE, "no graph uploaded");
	u64 const L(ctx->aligned_len);
	if (!(col_begin < col_end && col_end <= L))
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "column window [%llu, %llu) is empty or not within the aligned length %llu",
			(unsigned long long) col_begin, (unsigned long long) col_end, (unsigned long long) L);
	ctx->windowed = false;
	if (0 == col_begin && L == col_end) return V2M_OK;   // the whole row: the whole-row view and kernels
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	window_tile_tables tb;
	append_window_tiles(ctx, col_begin, col_end, tb);
	u32 const e_hi(tb.edge_end.back());
	tb.edge_begin.push_back(e_hi);       // (one window: edge_begin[t + 1] is the end of tile t's range)
	row_view &w(ctx->window);
	w.words = words_of_edges(ctx, first_edge_reaching_past(ctx, col_begin, e_hi), e_hi);
	w.begin = col_begin;
	w.end = col_end;
	w.max_unaligned = col_end - col_begin;   // a window's unaligned body never exceeds its columns
	w.n_tiles = u32(tb.edge_end.size());
	w.has_template0 = false;
	if (int const rc = upload_vec(ctx, w.d_edge_begin, tb.edge_begin)) return rc;
	if (int const rc = upload_vec(ctx, w.d_cross_offsets, tb.cross_offsets)) return rc;
	if (int const rc = upload_vec(ctx, w.d_cross_edges, tb.cross_edges)) return rc;
	if (int const rc = expand_reference(ctx, w, w.d_template, '-')) return rc;
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	ctx->windowed = true;
	return V2M_OK;
}


// ---- window sets ------------------------------------------------------------------------------------

int v2m_window_set_layout(uint64_t n_windows, const uint64_t *col_begin, const uint64_t *col_end, uint64_t *slot_offset, uint64_t *record_pitch)
{
	if (0 == n_windows) return fail(nullptr, V2M_ERR_INVALID_ARGUMENT, "a window set needs at least one window");
	if (!col_begin || !col_end) return fail(nullptr, V2M_ERR_INVALID_ARGUMENT, "NULL array");
	u64 at(0);
	for (u64 k(0); k < n_windows; ++k) {
		if (!(col_begin[k] < col_end[k]))
			return fail(nullptr, V2M_ERR_INVALID_ARGUMENT, "window %llu, [%llu, %llu), is empty", (unsigned long long) k, (unsigned long long) col_begin[k], (unsigned long long) col_end[k]);
		if (slot_offset) slot_offset[k] = at;
		u64 const len(col_end[k] - col_begin[k]);
		// (the unaligned kernels keep per-tile destinations in 32 bits; checked window by window, so that the sum cannot wrap either)
		if (len >= (u64(1) << 32) || (at += (len + 15) & ~u64(15)) >= (u64(1) << 32))
			return fail(nullptr, V2M_ERR_UNSUPPORTED, "the slots of the window set reach 2^32 bytes at window %llu: split the set", (unsigned long long) k);
	}
	if (record_pitch) *record_pitch = (at + 255) & ~u64(255);
	return V2M_OK;
}

uint64_t v2m_window_set_size(const v2m_ctx *ctx) { return (ctx && ctx->has_graph && ctx->has_set) ? ctx->set.n_windows : 0; }
uint64_t v2m_window_set_pitch(const v2m_ctx *ctx) { return (ctx && ctx->has_graph && ctx->has_set) ? ctx->set.pitch : 0; }

namespace {

// The REF row in the set's record layout with `gap` as padding (kernels.hpp: expand_reference_set_kernel): one launch over the tile
// table, one record long.
int expand_reference_set(v2m_ctx *ctx, dev_buf &dst, char gap)
{
	u64 const n_chunks(ctx->set.view.end / 16);
	V2M_HIP_TRY(ctx, dst.ensure(n_chunks * 16));
	{
		timed_launch tl(ctx, V2M_KERNEL_TEMPLATE);
		hipLaunchKernelGGL(v2m::expand_reference_set_kernel, dim3(unsigned((n_chunks + 255) / 256)), dim3(256), 0, ctx->stream,
			ctx->d_ref.as<char>(), ctx->d_ref_pos.as<u32>(), ctx->d_aln_pos.as<u32>(), u32(ctx->n_nodes), set_tables(ctx), ctx->set.view.n_tiles, n_chunks, dst.as<uint4>(), gap);
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	return V2M_OK;
}

struct scoped_set_call {
	v2m_ctx *ctx;
	explicit scoped_set_call(v2m_ctx *c) : ctx(c) { c->set_call = true; }
	~scoped_set_call() { ctx->set_call = false; }
};

int check_set_call(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags)
{
	if (int const rc = check_batch(ctx, rows, flags)) return rc;
	if (!ctx->has_set) return fail(ctx, V2M_ERR_STATE, "no window set (v2m_set_window_set)");
	if (flags & V2M_SPLICE_BGZF) return fail(ctx, V2M_ERR_UNSUPPORTED, "V2M_SPLICE_BGZF is not supported by the window-set calls");
	return V2M_OK;
}

} // namespace

int v2m_set_window_set(v2m_ctx *ctx, uint64_t n_windows, const uint64_t *col_begin, const uint64_t *col_end)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph) return fail(ctx, V2M_ERR_STATE, "no graph uploaded");
	if (0 == n_windows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "a window set needs at least one window");
	if (!col_begin || !col_end) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL array");
	u64 const L(ctx->aligned_len);
	u64 n_tiles(0);
	for (u64 k(0); k < n_windows; ++k) {
		if (!(col_begin[k] < col_end[k] && col_end[k] <= L))
			return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "window %llu, [%llu, %llu), is empty or not within the aligned length %llu",
				(unsigned long long) k, (unsigned long long) col_begin[k], (unsigned long long) col_end[k], (unsigned long long) L);
		n_tiles += (col_end[k] - col_begin[k] + v2m::kTileBytes - 1) / v2m::kTileBytes;
	}
	std::vector<u64> slot_offset(n_windows);
	u64 pitch(0);
	if (int const rc = v2m_window_set_layout(n_windows, col_begin, col_end, slot_offset.data(), &pitch)) return fail(ctx, rc, "%s", g_create_error.c_str());
	if (n_windows >= 0xFFFFFFFFull || n_tiles >= 0x7FFFFFFFull)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "the window set has too many tiles (%llu) for one set: split it", (unsigned long long) n_tiles);
	ctx->has_set = false;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	// The tiles of all windows in set order, each with its columns, its place in the record and its window; the resolve range is the
	// hull of the windows' ranges (a whole-row resolve is small beside the splice, so the hull costs nothing worth splitting).
	auto &set(ctx->set);
	window_tile_tables tb;
	std::vector<u32> tile_col_begin, tile_col_end, tile_record_offset, tile_window, first_tile(n_windows + 1), slot_offset32(n_windows);
	tile_col_begin.reserve(n_tiles); tile_col_end.reserve(n_tiles); tile_record_offset.reserve(n_tiles); tile_window.reserve(n_tiles);
	set.lengths.resize(n_windows);
	u64 e_lo(~u64(0)), e_hi(0), slots_end(0);
	for (u64 k(0); k < n_windows; ++k) {
		u64 const len(col_end[k] - col_begin[k]);
		first_tile[k] = tb.n_tiles();
		slot_offset32[k] = u32(slot_offset[k]);
		set.lengths[k] = u32(len);
		slots_end = slot_offset[k] + ((len + 15) & ~u64(15));
		append_window_tiles(ctx, col_begin[k], col_end[k], tb);
		for (u64 j(0); j * v2m::kTileBytes < len; ++j) {
			tile_col_begin.push_back(u32(col_begin[k] + j * v2m::kTileBytes));
			tile_col_end.push_back(u32(std::min<u64>(col_begin[k] + (j + 1) * v2m::kTileBytes, col_end[k])));
			tile_record_offset.push_back(u32(slot_offset[k] + j * v2m::kTileBytes));
			tile_window.push_back(u32(k));
		}
		u32 const w_hi(tb.edge_end.back());
		u64 const w_lo(first_edge_reaching_past(ctx, col_begin[k], w_hi));
		if (w_lo < w_hi) { e_lo = std::min(e_lo, w_lo); e_hi = std::max<u64>(e_hi, w_hi); }
	}
	first_tile[n_windows] = tb.n_tiles();
	tb.edge_begin.push_back(0);          // (tile_tables' [n_tiles + 1] shape; a set's range ends are edge_end)
	row_view &v(set.view);
	v.words = words_of_edges(ctx, std::min(e_lo, e_hi), e_hi);
	v.begin = 0;                         // the view's "columns" are a record's bytes
	v.end = slots_end;
	v.max_unaligned = slots_end;
	v.n_tiles = tb.n_tiles();
	v.has_template0 = false;
	set.n_windows = n_windows;
	set.pitch = pitch;
	u64 total(0);
	for (u32 const len : set.lengths) total += len;
	set.mean_tile_bytes = std::max<u64>(1, total / v.n_tiles);
	if (int const rc = upload_vec(ctx, v.d_edge_begin, tb.edge_begin)) return rc;
	if (int const rc = upload_vec(ctx, v.d_cross_offsets, tb.cross_offsets)) return rc;
	if (int const rc = upload_vec(ctx, v.d_cross_edges, tb.cross_edges)) return rc;
	if (int const rc = upload_vec(ctx, set.d_edge_end, tb.edge_end)) return rc;
	if (int const rc = upload_vec(ctx, set.d_col_begin, tile_col_begin)) return rc;
	if (int const rc = upload_vec(ctx, set.d_col_end, tile_col_end)) return rc;
	if (int const rc = upload_vec(ctx, set.d_record_offset, tile_record_offset)) return rc;
	if (int const rc = upload_vec(ctx, set.d_tile_window, tile_window)) return rc;
	if (int const rc = upload_vec(ctx, set.d_first_tile, first_tile)) return rc;
	if (int const rc = upload_vec(ctx, set.d_slot_offset32, slot_offset32)) return rc;
	if (int const rc = expand_reference_set(ctx, v.d_template, '-')) return rc;
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the uploads read this call's vectors)
	ctx->has_set = true;
	return V2M_OK;
}

int v2m_splice_window_set(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_window_sink_fn sink, void *user)
{
	if (int const rc = check_set_call(ctx, rows, flags)) return rc;
	if (!sink) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "sink is NULL");
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	scoped_set_call const in_set(ctx);
	u64 const n_windows(ctx->set.n_windows);
	return splice_rows_pipeline(ctx, rows, flags & V2M_SPLICE_UNALIGNED, 2, "v2m_splice_window_set", [&](v2m_row_hold &, slot_rows const &sl) -> int {
		for (u64 r(sl.r0); r < sl.r1; ++r)
			if (sink(user, r, sl.row(r), sl.set_lengths ? sl.set_lengths + (r - sl.r0) * n_windows : ctx->set.lengths.data()))
				return fail(ctx, V2M_ERR_SINK, "sink aborted at row %llu", (unsigned long long) r);
		return V2M_OK;
	});
}

int v2m_splice_window_set_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_out, uint64_t record_pitch, uint32_t *lengths_out)
{
	if (int const rc = check_set_call(ctx, rows, flags)) return rc;
	if (0 == rows->n_rows) return V2M_OK;
	if (!d_out || ((uintptr_t) d_out & 15)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_out must be a 16-byte aligned device pointer");
	if (record_pitch % 16 || record_pitch < ctx->set.view.end)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "record_pitch must be a multiple of 16 and at least the end of the last slot, %llu", (unsigned long long) ctx->set.view.end);
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	scoped_set_call const in_set(ctx);
	u64 const n_windows(ctx->set.n_windows);
	if (!(flags & V2M_SPLICE_UNALIGNED)) {
		if (int const rc = splice_aligned_slice(ctx, rows, 0, rows->n_rows, static_cast<char *>(d_out), record_pitch)) return rc;
		if (lengths_out)
			for (u64 r(0); r < rows->n_rows; ++r) std::copy(ctx->set.lengths.begin(), ctx->set.lengths.end(), lengths_out + r * n_windows);
		return V2M_OK;
	}
	ctx->set_lengths_slot = 0;
	if (int const rc = splice_unaligned_slice(ctx, rows, 0, rows->n_rows, static_cast<char *>(d_out), record_pitch)) return rc;
	if (lengths_out) {
		V2M_HIP_TRY(ctx, hipMemcpyAsync(lengths_out, ctx->d_set_lengths[0].p, rows->n_rows * n_windows * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	return V2M_OK;
}


// ---- distinct pieces of a window set ----------------------------------------------------------------

namespace {

u64 env_u64(char const *name, u64 fallback)
{
	char const *const e(std::getenv(name));
	return (e && *e) ? std::strtoull(e, nullptr, 10) : fallback;
}

// A class of one window: its first row, its bytes' place in the pool, its number within the window (given when its slice is done)
// and the next class of the same window with the same key and length (a key collision).
struct distinct_class {
	u64 first_row, pool_offset;
	u32 window, length, index, next;
};

struct distinct_key {
	u64 key;
	u32 window, length;
	bool operator==(distinct_key const &o) const { return key == o.key && window == o.window && length == o.length; }
};

struct distinct_key_hash {
	std::size_t operator()(distinct_key const &k) const { return std::size_t(v2m::mix64(k.key ^ (u64(k.window) << 32 | k.length) * v2m::kGolden)); }
};

constexpr u32 kNoClass = ~u32(0);

// The slices of the set calls, with the records staying in the device slot: per slice the keys of its pieces come to the host, which
// looks every piece up per (window, key, length) in a table that lives for the call -- a piece with an unknown key becomes a class's
// representative and is gathered into the pool, every other piece is verified byte for byte against its candidate's pool entry; a
// mismatch (a key collision) moves the piece on to the next class with that key, or makes it a representative in the next round.
// The classes a slice has added leave for the host in one copy of the slice's pool bytes on the copy stream, and are handed to the
// sink while the next slice's kernels run.
int distinct_run(v2m_ctx *ctx, v2m_row_batch const *rows, bool unaligned, v2m_distinct_sink_fn sink, void *user, u32 *class_of_out, u32 *n_classes_out)
{
	auto const &set(ctx->set);
	u64 const W(set.n_windows), n_rows(rows->n_rows);
	u64 const hash_bits(std::min<u64>(64, env_u64("V2M_DISTINCT_HASH_BITS", 64)));   // test knob: fewer bits, more collisions, the same classes
	u64 const key_mask(hash_bits >= 64 ? ~u64(0) : (u64(1) << hash_bits) - 1);
	std::size_t free_bytes(0), total_bytes(0);
	V2M_HIP_TRY(ctx, hipMemGetInfo(&free_bytes, &total_bytes));
	u64 const pool_limit(std::min<u64>(env_u64("V2M_DISTINCT_POOL_BYTES", u64(4) << 30), free_bytes));

	// the items of a row in hash_pieces_kernel, and the windows' lengths for aligned mode
	std::vector<u32> window_table(2 * W + 1);
	std::vector<u64> slot_offset(W);
	u64 items_per_row(0), slots_end(0);
	for (u64 k(0); k < W; ++k) {
		window_table[k] = u32(items_per_row);
		u32 const len(set.lengths[k]);
		slot_offset[k] = slots_end;
		slots_end += (u64(len) + 15) & ~u64(15);
		items_per_row += len <= v2m::kDistinctLongBytes ? 1 : (len + v2m::kDistinctChunkBytes - 1) / v2m::kDistinctChunkBytes;
		window_table[W + 1 + k] = len;
	}
	if (items_per_row >= 0xFFFFFFFFull) return fail(ctx, V2M_ERR_UNSUPPORTED, "the window set has too many chunks (%llu) for one set: split it", (unsigned long long) items_per_row);
	window_table[W] = u32(items_per_row);
	if (int const rc = upload_vec(ctx, ctx->d_distinct_windows, window_table)) return rc;
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // (the upload reads this call's vector)
	u32 const *const d_first_item(ctx->d_distinct_windows.as<u32>());
	u32 const *const d_window_lengths(d_first_item + W + 1);

	// per piece 8 bytes of key and 4 of length, and a round's item (24) and flag (4)
	slice_plan const p(plan_slices(ctx, n_rows, unaligned, ~u64(0), 40 * W));
	if (int const rc = ensure_host_slots(ctx, 2, 0)) return rc;

	std::vector<distinct_class> classes;
	std::unordered_map<distinct_key, u32, distinct_key_hash> heads;
	std::vector<u32> n_classes(W, 0);
	scratch_buf pool;
	u64 pool_used(0);
	struct delivery { std::vector<u32> ids; u64 pool_begin{}; bool pending{}; } deliveries[2];

	auto const grow_pool([&](u64 keep) -> int {
		if (pool_used > pool_limit)
			return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "the distinct pieces need %llu bytes so far, more than the pool may hold: V2M_DISTINCT_POOL_BYTES is %llu (default 4 GiB, clamped to the free device memory)",
				(unsigned long long) pool_used, (unsigned long long) pool_limit);
		if (pool_used <= pool.bytes) return V2M_OK;
		scratch_buf bigger;
		V2M_HIP_TRY(ctx, bigger.dev_buf::ensure(std::min(pool_limit, std::max<u64>({pool_used, 2 * u64(pool.bytes), u64(1) << 20}))));
		if (keep) {
			V2M_HIP_TRY(ctx, hipMemcpyAsync(bigger.p, pool.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		}
		std::swap(pool.p, bigger.p);
		std::swap(pool.bytes, bigger.bytes);
		return V2M_OK;
	});

	auto const deliver([&](delivery &d, v2m_row_hold &slot) -> int {
		if (!d.pending) return V2M_OK;
		d.pending = false;
		V2M_HIP_TRY(ctx, hipEventSynchronize(slot.copied));
		char const *const base(slot.host.as<char>());
		for (u32 const id : d.ids) {
			distinct_class const &c(classes[id]);
			if (sink(user, c.window, c.index, c.first_row, c.length ? base + (c.pool_offset - d.pool_begin) : "", c.length))
				return fail(ctx, V2M_ERR_SINK, "sink aborted at class %u of window %u", c.index, c.window);
		}
		return V2M_OK;
	});

	auto const push_items([&](std::vector<v2m::piece_item> &items, u64 src, u64 dst, u32 len, u32 index) {
		for (u32 at(0); at < len; at += v2m::kDistinctChunkBytes)
			items.push_back({src + at, dst + at, std::min(v2m::kDistinctChunkBytes, len - at), index});
	});

	std::vector<u32> piece_class, pending, next_pending, pair_piece, slice_new;
	std::vector<v2m::piece_item> gather_items, verify_items;

	auto const slice([&](u64 s) -> int {
		u64 const r0(s * p.rows_per_slice), r1(std::min(n_rows, r0 + p.rows_per_slice)), nr(r1 - r0), n_pieces(nr * W);
		V2M_HIP_TRY(ctx, ctx->ring[0].ensure(p.slot_bytes));   // (the slice takes its device slot: refilled in the checked build)
		char *const d_records(ctx->ring[0].as<char>());
		ctx->set_lengths_slot = 0;
		if (int const rc = unaligned ? splice_unaligned_slice(ctx, rows, r0, r1, d_records, p.pitch) : splice_aligned_slice(ctx, rows, r0, r1, d_records, p.pitch))
			return rc;
		V2M_HIP_TRY(ctx, ctx->d_distinct_keys.ensure(n_pieces * 8));
		V2M_HIP_TRY(ctx, hipMemsetAsync(ctx->d_distinct_keys.p, 0, n_pieces * 8, ctx->stream));
		u32 const *const d_lengths(unaligned ? ctx->d_set_lengths[0].as<u32>() : d_window_lengths);
		{
			timed_launch tl(ctx, V2M_KERNEL_DISTINCT_HASH);
			u64 const rows_per_launch(32768);   // (the grid's y)
			for (u64 b(0); b < nr; b += rows_per_launch) {
				u64 const n(std::min(rows_per_launch, nr - b));
				hipLaunchKernelGGL(v2m::hash_pieces_kernel, dim3(unsigned((items_per_row + v2m::kDistinctWaves - 1) / v2m::kDistinctWaves), unsigned(n)), dim3(v2m::kDistinctThreads), 0, ctx->stream,
					d_records + b * p.pitch, p.pitch, u32(W), set.d_slot_offset32.as<u32>(), unaligned ? d_lengths + b * W : d_lengths, unaligned ? u32(W) : 0u,
					d_first_item, ctx->d_distinct_keys.as<unsigned long long>() + b * W);
			}
		}
		V2M_HIP_TRY(ctx, hipGetLastError());
		V2M_HIP_TRY(ctx, ctx->h_distinct_keys.ensure(n_pieces * 12));
		V2M_POISON_HOST(ctx->h_distinct_keys.p, n_pieces * 12);
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_distinct_keys.p, ctx->d_distinct_keys.p, n_pieces * 8, hipMemcpyDeviceToHost, ctx->stream));
		if (unaligned)
			V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_distinct_keys.as<char>() + n_pieces * 8, d_lengths, n_pieces * 4, hipMemcpyDeviceToHost, ctx->stream));
		// the previous slice's classes go to the sink under this slice's kernels
		if (s >= 1) if (int const rc = deliver(deliveries[(s - 1) & 1], *ctx->host_slots[(s - 1) & 1])) return rc;
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		u64 const *const keys(ctx->h_distinct_keys.as<u64>());
		u32 const *const slice_lengths(reinterpret_cast<u32 const *>(ctx->h_distinct_keys.as<char>() + n_pieces * 8));
		auto const length_of([&](u64 i) { return unaligned ? slice_lengths[i] : set.lengths[i % W]; });
		auto const record_offset([&](u64 i) { return (i / W) * p.pitch + slot_offset[i % W]; });

		u64 const slice_pool_begin(pool_used);
		piece_class.assign(n_pieces, kNoClass);
		slice_new.clear();
		pending.clear();
		auto const new_class([&](u64 i, u32 len) -> u32 {
			u32 const id(u32(classes.size()));
			classes.push_back({r0 + i / W, pool_used, u32(i % W), len, 0, kNoClass});
			if (len) push_items(gather_items, record_offset(i), pool_used, len, 0);
			pool_used += (u64(len) + 15) & ~u64(15);
			slice_new.push_back(id);
			piece_class[i] = id;
			return id;
		});
		auto const try_class([&](u64 i, u32 len, u32 candidate) {
			piece_class[i] = candidate;
			if (0 == len) return;   // (all empty pieces of a window are one class)
			push_items(verify_items, record_offset(i), classes[candidate].pool_offset, len, u32(pair_piece.size()));
			pair_piece.push_back(u32(i));
		});
		for (u64 round(0);; ++round) {
			gather_items.clear(); verify_items.clear(); pair_piece.clear();
			u64 const round_pool_begin(pool_used);
			if (0 == round) {
				for (u64 i(0); i < n_pieces; ++i) {
					u32 const len(length_of(i));
					auto const found(heads.find({keys[i] & key_mask, u32(i % W), len}));
					if (heads.end() == found) heads.insert({{keys[i] & key_mask, u32(i % W), len}, new_class(i, len)});
					else try_class(i, len, found->second);
				}
			}
			else {
				for (u32 const i : pending) {   // in piece order: an earlier piece of the same bytes becomes the representative first
					u32 const len(length_of(i));
					u32 const tried(piece_class[i]);
					if (kNoClass == classes[tried].next) { u32 const id(new_class(i, len)); classes[tried].next = id; }
					else try_class(i, len, classes[tried].next);
				}
			}
			if (classes.size() >= kNoClass) return fail(ctx, V2M_ERR_UNSUPPORTED, "too many distinct pieces in one call");
			if (int const rc = grow_pool(round_pool_begin)) return rc;
			if (verify_items.empty() && gather_items.empty()) break;
			u64 const n_gather(gather_items.size()), n_verify(verify_items.size()), n_pairs(pair_piece.size());
			V2M_HIP_TRY(ctx, ctx->h_distinct_items.ensure((n_gather + n_verify) * sizeof(v2m::piece_item)));
			V2M_HIP_TRY(ctx, ctx->d_distinct_items.ensure((n_gather + n_verify) * sizeof(v2m::piece_item)));
			v2m::piece_item *const h_items(ctx->h_distinct_items.as<v2m::piece_item>());
			std::copy(gather_items.begin(), gather_items.end(), h_items);
			std::copy(verify_items.begin(), verify_items.end(), h_items + n_gather);
			V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_distinct_items.p, h_items, (n_gather + n_verify) * sizeof(v2m::piece_item), hipMemcpyHostToDevice, ctx->stream));
			v2m::piece_item const *const d_items(ctx->d_distinct_items.as<v2m::piece_item>());
			if (n_gather) {
				timed_launch tl(ctx, V2M_KERNEL_DISTINCT_GATHER);
				for (u64 b(0); b < n_gather; b += u64(1) << 32) {
					u64 const n(std::min<u64>(u64(1) << 32, n_gather - b));
					hipLaunchKernelGGL(v2m::gather_pieces_kernel, dim3(unsigned((n + v2m::kDistinctWaves - 1) / v2m::kDistinctWaves)), dim3(v2m::kDistinctThreads), 0, ctx->stream,
						d_records, d_items + b, n, pool.as<char>());
				}
			}
			if (n_verify) {
				V2M_HIP_TRY(ctx, ctx->d_distinct_flags.ensure(n_pairs * 4));
				V2M_HIP_TRY(ctx, ctx->h_distinct_flags.ensure(n_pairs * 4));
				V2M_POISON_HOST(ctx->h_distinct_flags.p, n_pairs * 4);
				V2M_HIP_TRY(ctx, hipMemsetAsync(ctx->d_distinct_flags.p, 0, n_pairs * 4, ctx->stream));
				{
					timed_launch tl(ctx, V2M_KERNEL_DISTINCT_VERIFY);
					for (u64 b(0); b < n_verify; b += u64(1) << 32) {
						u64 const n(std::min<u64>(u64(1) << 32, n_verify - b));
						hipLaunchKernelGGL(v2m::verify_pieces_kernel, dim3(unsigned((n + v2m::kDistinctWaves - 1) / v2m::kDistinctWaves)), dim3(v2m::kDistinctThreads), 0, ctx->stream,
							d_records, pool.as<char>(), d_items + n_gather + b, n, ctx->d_distinct_flags.as<u32>());
					}
				}
				V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_distinct_flags.p, ctx->d_distinct_flags.p, n_pairs * 4, hipMemcpyDeviceToHost, ctx->stream));
			}
			V2M_HIP_TRY(ctx, hipGetLastError());
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			next_pending.clear();
			u32 const *const flags(ctx->h_distinct_flags.as<u32>());
			for (u64 j(0); j < n_pairs; ++j) if (flags[j]) next_pending.push_back(pair_piece[j]);
			pending.swap(next_pending);
			if (pending.empty()) break;
		}

		// the slice's classes in the order of their first rows (a later round's class may begin before an earlier round's): their numbers
		std::sort(slice_new.begin(), slice_new.end(), [&](u32 a, u32 b) {
			return classes[a].first_row != classes[b].first_row ? classes[a].first_row < classes[b].first_row : classes[a].window < classes[b].window; });
		for (u32 const id : slice_new) classes[id].index = n_classes[classes[id].window]++;
		for (u64 i(0); i < n_pieces; ++i) class_of_out[r0 * W + i] = classes[piece_class[i]].index;
		if (sink && !slice_new.empty()) {
			delivery &d(deliveries[s & 1]);
			v2m_row_hold &slot(*ctx->host_slots[s & 1]);
			u64 const bytes(pool_used - slice_pool_begin);
			V2M_HIP_TRY(ctx, slot.host.ensure(bytes));
			V2M_POISON_HOST(slot.host.p, bytes);
			if (bytes) V2M_HIP_TRY(ctx, hipMemcpyAsync(slot.host.p, pool.as<char>() + slice_pool_begin, bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
			V2M_HIP_TRY(ctx, hipEventRecord(slot.copied, ctx->copy_stream));
			d.ids = slice_new;
			d.pool_begin = slice_pool_begin;
			d.pending = true;
		}
		return V2M_OK;
	});

	int rc(V2M_OK);
	for (u64 s(0); s < p.n_slices && V2M_OK == rc; ++s) rc = slice(s);
	if (V2M_OK == rc && p.n_slices) rc = deliver(deliveries[(p.n_slices - 1) & 1], *ctx->host_slots[(p.n_slices - 1) & 1]);
	// leave both streams idle whatever happened (the pool goes with the call)
	(void) hipStreamSynchronize(ctx->stream);
	(void) hipStreamSynchronize(ctx->copy_stream);
	if (V2M_OK == rc && n_classes_out) std::copy(n_classes.begin(), n_classes.end(), n_classes_out);
	return rc;
}

} // namespace

int v2m_splice_window_set_distinct(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_distinct_sink_fn sink, void *user, uint32_t *class_of_out, uint32_t *n_classes_out)
{
	if (int const rc = check_set_call(ctx, rows, flags)) return rc;
	if (!class_of_out) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "class_of_out is NULL");
	if (n_classes_out) std::fill(n_classes_out, n_classes_out + ctx->set.n_windows, 0u);
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	scoped_set_call const in_set(ctx);
	return distinct_run(ctx, rows, flags & V2M_SPLICE_UNALIGNED, sink, user, class_of_out, n_classes_out);
}


// ---- founder search: chunk walks ------------------------------------------------------------------

namespace {

// What both founder entry points ask of the ctx and of their start states, and the edge-major bits they walk.
int pbwt_check_state(v2m_ctx *ctx, uint64_t n_copies, uint64_t n_chunks, const uint32_t *start_order, int max_copies)
{
	if (0 == n_copies || n_copies > u64(max_copies)) return fail(ctx, V2M_ERR_UNSUPPORTED, "this GPU chunk walk holds at most %d chromosome copies (got %llu)", max_copies, (unsigned long long) n_copies);
	if (n_copies > ctx->path_cols) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "the bound path matrix has %llu copies, %llu asked for", (unsigned long long) ctx->path_cols, (unsigned long long) n_copies);
	// (the kernels stage a whole edge column -- path_cols / 64 words -- in an LDS array sized with the state)
	if (ctx->path_cols > u64(max_copies)) return fail(ctx, V2M_ERR_UNSUPPORTED, "this GPU chunk walk reads edge columns of at most %d copies; the bound path matrix has %llu columns", max_copies, (unsigned long long) ctx->path_cols);
	// (biased divergence values are edge indices + 2, and the kernels keep bit 31 of a running maximum for "constant")
	if (ctx->n_edges >= 0x7FFFFFF0ull) return fail(ctx, V2M_ERR_UNSUPPORTED, "the GPU chunk walk keeps edge indices in 31 bits (the graph has %llu edges)", (unsigned long long) ctx->n_edges);
	// the start order indexes the workgroup's state arrays in LDS
	for (u64 i(0), n(n_chunks * n_copies); i < n; ++i)
		if (start_order[i] >= n_copies) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "start_order[%llu] = %u is not a chromosome copy (%llu copies)", (unsigned long long) i, start_order[i], (unsigned long long) n_copies);
	return V2M_OK;
}

int edge_major_paths(v2m_ctx *ctx, u64 const **d_by_edge_out)
{
	u64 const rows(ctx->path_rows), cols(ctx->path_cols);              // both multiples of 64
	if (!ctx->by_edge_valid) {
		V2M_HIP_TRY(ctx, ctx->d_by_edge.ensure(std::max<size_t>(16, rows * (cols / 64) * sizeof(u64))));
		if (int const rc = launch_transpose(ctx, ctx->d_paths, rows, cols, ctx->d_by_edge.as<u64>(), ctx->path_pitch, 0)) return rc;
		ctx->by_edge_valid = true;
	}
	*d_by_edge_out = ctx->d_by_edge.as<u64>();
	return V2M_OK;
}

// v2m_pbwt_cut_trials (the pairs land in the caller's arrays) and v2m_pbwt_cut_trials_streamed (they pass through two pinned
// slots and a callback takes them chunk by chunk while the next slice is on its way).
int pbwt_cut_trials_impl(v2m_ctx *ctx, uint64_t n_copies, uint64_t min_distance,
	uint64_t n_candidates, const uint32_t *cand_edge, const uint64_t *cand_aligned_pos,
	uint64_t n_chunks, const uint64_t *chunk_first, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t trial_capacity, uint32_t *trial_pred, uint32_t *trial_class_count, uint64_t *trial_end, uint32_t *chunk_status,
	v2m_trials_sink sink, void *sink_user)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph || !ctx->d_paths) return fail(ctx, V2M_ERR_STATE, "the founder search needs an uploaded graph with its path matrix");
	if (0 == n_chunks) return V2M_OK;
	if (!cand_edge || !cand_aligned_pos || !chunk_first || !start_order || !start_divergence || (!sink && (!trial_pred || !trial_class_count)) || !trial_end || !chunk_status)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL array");
	if (int const rc = pbwt_check_state(ctx, n_copies, n_chunks, start_order, v2m::kPbwtMaxCopies)) return rc;
	if (n_candidates >= 0xFFFFFFFFull || ctx->n_edges >= 0xFFFFFFFDull) return fail(ctx, V2M_ERR_UNSUPPORTED, "candidate and edge indices are kept in 32 bits");
	if (chunk_first[0] < 1 || chunk_first[n_chunks] > n_candidates) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "chunk bounds outside the candidate list");
	for (u64 k(0); k < n_chunks; ++k) if (chunk_first[k] > chunk_first[k + 1]) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "chunk bounds must not decrease");
	// the candidates as find_cut_positions.cc:113,126-151 makes them: the sentinel (edge 0, node 0), then one per distinct edge index in
	// node order -- both columns ascend (the first real candidate may share edge 0 with the sentinel)
	for (u64 c(0); c < n_candidates; ++c) {
		if (cand_edge[c] > ctx->n_edges || (c && cand_edge[c] < cand_edge[c - 1])) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "candidate edges must ascend and stay inside the graph (candidate %llu)", (unsigned long long) c);
		if (c && cand_aligned_pos[c] < cand_aligned_pos[c - 1]) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "candidate aligned positions must not decrease (candidate %llu)", (unsigned long long) c);
	}
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	// edge-major bits: the bound matrix (rows = edges, columns = copies) transposed back on the device, once per binding
	u64 const cols(ctx->path_cols);
	u64 const *d_by_edge(nullptr);
	if (int const rc = edge_major_paths(ctx, &d_by_edge)) return rc;
	dev_buf d_first, d_cand_edge, d_cand_aln, d_chunk_first, d_order, d_div, d_pred, d_class, d_end, d_status;

	auto const up([&](dev_buf &dst, void const *src, size_t bytes) -> int {
		V2M_HIP_TRY(ctx, dst.ensure(std::max<size_t>(bytes, 16)));
		if (bytes) V2M_HIP_TRY(ctx, hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
		return V2M_OK;
	});
	if (int const rc = up(d_cand_edge, cand_edge, n_candidates * sizeof(u32))) return rc;
	if (int const rc = up(d_cand_aln, cand_aligned_pos, n_candidates * sizeof(u64))) return rc;
	if (int const rc = up(d_chunk_first, chunk_first, (n_chunks + 1) * sizeof(u64))) return rc;
	if (int const rc = up(d_order, start_order, n_chunks * n_copies * sizeof(u32))) return rc;
	if (int const rc = up(d_div, start_divergence, n_chunks * n_copies * sizeof(u32))) return rc;
	u32 const n_edges(u32(ctx->n_edges));
	V2M_HIP_TRY(ctx, d_first.ensure((u64(n_edges) + 1) * sizeof(u32)));
	V2M_HIP_TRY(ctx, d_pred.ensure(std::max<u64>(16, n_chunks * trial_capacity * sizeof(u32))));
	V2M_HIP_TRY(ctx, d_class.ensure(std::max<u64>(16, n_chunks * trial_capacity * sizeof(u32))));
	V2M_HIP_TRY(ctx, d_end.ensure(n_candidates * sizeof(u64)));
	V2M_HIP_TRY(ctx, d_status.ensure(n_chunks * sizeof(u32)));
	V2M_HIP_TRY(ctx, hipMemsetAsync(d_status.p, 0xFF, n_chunks * sizeof(u32), ctx->stream));
	hipLaunchKernelGGL(v2m::pbwt_first_candidate_kernel, dim3(unsigned((u64(n_edges) + 1 + 255) / 256)), dim3(256), 0, ctx->stream,
		d_cand_edge.as<u32>(), u32(n_candidates), n_edges, d_first.as<u32>());
	// (the kernel is instantiated per copies-per-thread count, 1 .. 8, so that its per-copy loops unroll without branches)
	auto const launch_trials([&](auto per_tag) {
		hipLaunchKernelGGL((v2m::pbwt_cut_trials_kernel<decltype(per_tag)::value>), dim3(unsigned(n_chunks)), dim3(v2m::kPbwtThreads), 0, ctx->stream,
			d_by_edge, u32(cols / 64), u32(n_copies), n_edges, d_first.as<u32>(), d_cand_edge.as<u32>(), d_cand_aln.as<u64>(), min_distance,
			d_chunk_first.as<u64>(), d_order.as<u32>(), d_div.as<u32>(), trial_capacity, d_pred.as<u32>(), d_class.as<u32>(), d_end.as<u64>(), d_status.as<u32>());
	});
	pbwt_dispatch_per_thread<v2m::kPbwtPerThread>(ctx->path_cols, launch_trials);
	V2M_HIP_TRY(ctx, hipGetLastError());
	V2M_HIP_TRY(ctx, hipMemcpyAsync(chunk_status, d_status.p, n_chunks * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
	// (only the candidates of this call's chunks: a caller may be consuming an earlier call's part of the same array meanwhile)
	u64 const cand_lo(chunk_first[0]), cand_hi(chunk_first[n_chunks]);
	if (cand_hi > cand_lo) V2M_HIP_TRY(ctx, hipMemcpyAsync(trial_end + cand_lo, d_end.as<u64>() + cand_lo, (cand_hi - cand_lo) * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	// only what the chunks produced comes back
	std::vector<u64> produced(n_chunks, 0);
	for (u64 k(0); k < n_chunks; ++k) {
		if (0 != chunk_status[k] || chunk_first[k] == chunk_first[k + 1]) { if (0 != chunk_status[k]) chunk_status[k] = 1; continue; }
		u64 const n(trial_end[chunk_first[k + 1] - 1]);
		if (n > trial_capacity) { chunk_status[k] = 1; continue; }
		produced[k] = n;
	}
	if (!sink) {
		for (u64 k(0); k < n_chunks; ++k) {
			if (0 == produced[k]) continue;
			V2M_HIP_TRY(ctx, hipMemcpyAsync(trial_pred + k * trial_capacity, d_pred.as<u32>() + k * trial_capacity, produced[k] * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
			V2M_HIP_TRY(ctx, hipMemcpyAsync(trial_class_count + k * trial_capacity, d_class.as<u32>() + k * trial_capacity, produced[k] * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
		}
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		return V2M_OK;
	}

	// Streamed: runs of whole chunks travel through two pinned slots in turn (pairs of a slice: preds first, class counts behind them); while
	// the callback works through one slice the next one crosses the link.  Nothing of the caller's is ever the target of a copy:
	// hundreds of MB of pageable memory as a copy target cost more to fault in, pin and release than the pairs take to use.
	u64 const slot_pairs(std::max<u64>(trial_capacity, u64(4) << 20));
	for (auto &slot : ctx->trials_stage) V2M_HIP_TRY(ctx, slot.ensure(2 * slot_pairs * sizeof(u32)));
	scoped_events ev;
	V2M_HIP_TRY(ctx, ev.create(2));
	struct slice { u64 first, end; };
	std::vector<slice> slices;
	for (u64 k(0); k < n_chunks;) {
		u64 end(k), pairs(0);
		while (end < n_chunks && (end == k || pairs + produced[end] <= slot_pairs)) pairs += produced[end++];
		slices.push_back({k, end});
		k = end;
	}
	auto const issue([&](std::size_t i) -> int {
		u32 *const pred(ctx->trials_stage[i & 1].as<u32>()), *const cls(pred + slot_pairs);
		V2M_POISON_HOST(pred, 2 * slot_pairs * sizeof(u32));
		u64 at(0);
		for (u64 k(slices[i].first); k < slices[i].end; ++k) {
			if (0 == produced[k]) continue;
			V2M_HIP_TRY(ctx, hipMemcpyAsync(pred + at, d_pred.as<u32>() + k * trial_capacity, produced[k] * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
			V2M_HIP_TRY(ctx, hipMemcpyAsync(cls + at, d_class.as<u32>() + k * trial_capacity, produced[k] * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
			at += produced[k];
		}
		V2M_HIP_TRY(ctx, hipEventRecord(ev[i & 1], ctx->stream));
		return V2M_OK;
	});
	if (int const rc = issue(0)) return rc;
	for (std::size_t i(0); i < slices.size(); ++i) {
		if (i + 1 < slices.size()) if (int const rc = issue(i + 1)) return rc;          // (the other slot: slice i - 1 has been handed over)
		V2M_HIP_TRY(ctx, hipEventSynchronize(ev[i & 1]));
		u32 const *const pred(ctx->trials_stage[i & 1].as<u32>()), *const cls(pred + slot_pairs);
		u64 at(0);
		for (u64 k(slices[i].first); k < slices[i].end; ++k) {
			if (int const rc = sink(sink_user, k, chunk_status[k], pred + at, cls + at, produced[k])) {
				(void) hipStreamSynchronize(ctx->stream);
				return fail(ctx, V2M_ERR_SINK, "the trial sink returned %d at chunk %llu", rc, (unsigned long long) k);
			}
			at += produced[k];
		}
	}
	return V2M_OK;
}

} // namespace


int v2m_pbwt_cut_trials(v2m_ctx *ctx, uint64_t n_copies, uint64_t min_distance,
	uint64_t n_candidates, const uint32_t *cand_edge, const uint64_t *cand_aligned_pos,
	uint64_t n_chunks, const uint64_t *chunk_first, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t trial_capacity, uint32_t *trial_pred, uint32_t *trial_class_count, uint64_t *trial_end, uint32_t *chunk_status)
{
	return pbwt_cut_trials_impl(ctx, n_copies, min_distance, n_candidates, cand_edge, cand_aligned_pos, n_chunks, chunk_first, start_order, start_divergence,
		trial_capacity, trial_pred, trial_class_count, trial_end, chunk_status, nullptr, nullptr);
}


int v2m_pbwt_cut_trials_streamed(v2m_ctx *ctx, uint64_t n_copies, uint64_t min_distance,
	uint64_t n_candidates, const uint32_t *cand_edge, const uint64_t *cand_aligned_pos,
	uint64_t n_chunks, const uint64_t *chunk_first, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t trial_capacity, uint64_t *trial_end, uint32_t *chunk_status, v2m_trials_sink sink, void *sink_user)
{
	if (ctx && !sink) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL sink");
	return pbwt_cut_trials_impl(ctx, n_copies, min_distance, n_candidates, cand_edge, cand_aligned_pos, n_chunks, chunk_first, start_order, start_divergence,
		trial_capacity, nullptr, nullptr, trial_end, chunk_status, sink, sink_user);
}


int v2m_pbwt_cut_records(v2m_ctx *ctx, uint64_t n_copies, uint64_t n_cuts, const uint32_t *cut_edge,
	uint64_t n_chunks, const uint64_t *chunk_first_cut, const uint32_t *start_edge, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t pool_capacity, uint32_t *pool_lhs, uint32_t *pool_rhs, uint32_t *pool_size,
	uint64_t *rec_pool_end, uint32_t *rec_distinct, uint32_t *rec_first_class, uint32_t *rec_first_is_ref, uint32_t *chunk_status)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!ctx->has_graph || !ctx->d_paths) return fail(ctx, V2M_ERR_STATE, "the founder search needs an uploaded graph with its path matrix");
	if (0 == n_chunks) return V2M_OK;
	if (!cut_edge || !chunk_first_cut || !start_edge || !start_order || !start_divergence || !pool_lhs || !pool_rhs || !pool_size
		|| !rec_pool_end || !rec_distinct || !rec_first_class || !rec_first_is_ref || !chunk_status)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "NULL array");
	if (int const rc = pbwt_check_state(ctx, n_copies, n_chunks, start_order, v2m::kPbwtMaxCopiesRecords)) return rc;
	if (chunk_first_cut[0] < 1 || chunk_first_cut[n_chunks] > n_cuts) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "chunk bounds outside the cut list");
	for (u64 k(0); k < n_chunks; ++k) {
		if (chunk_first_cut[k] > chunk_first_cut[k + 1]) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "chunk bounds must not decrease");
		if (chunk_first_cut[k] < chunk_first_cut[k + 1] && start_edge[k] > cut_edge[chunk_first_cut[k] - 1]) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "chunk %llu: the start state lies past the cut before its first one", (unsigned long long) k);
	}
	for (u64 j(0); j < n_cuts; ++j) if ((j && cut_edge[j] < cut_edge[j - 1]) || cut_edge[j] > ctx->n_edges) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "cut edges must ascend and stay inside the graph");
	// (no edge in a two-block span: no copy starts a joined class there, and the reference stops at its libbio_assert(!joined_path_eq_classes.empty()), :245)
	for (u64 j(2); j < n_cuts; ++j) if (cut_edge[j] == cut_edge[j - 2]) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "cuts %llu to %llu have no ALT edge between them: the two-block span that ends at cut %llu has no path classes", (unsigned long long) (j - 2), (unsigned long long) j, (unsigned long long) j);
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	u64 const rows(ctx->path_rows), cols(ctx->path_cols);
	u64 const *d_by_edge(nullptr);
	if (int const rc = edge_major_paths(ctx, &d_by_edge)) return rc;
	dev_buf d_cut_edge, d_chunk_first, d_start_edge, d_order, d_div, d_lhs, d_rhs, d_size, d_end, d_distinct, d_first, d_ref, d_status;
	auto const up([&](dev_buf &dst, void const *src, size_t bytes) -> int {
		V2M_HIP_TRY(ctx, dst.ensure(std::max<size_t>(bytes, 16)));
		if (bytes) V2M_HIP_TRY(ctx, hipMemcpyAsync(dst.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
		return V2M_OK;
	});
	if (int const rc = up(d_cut_edge, cut_edge, n_cuts * sizeof(u32))) return rc;
	if (int const rc = up(d_chunk_first, chunk_first_cut, (n_chunks + 1) * sizeof(u64))) return rc;
	if (int const rc = up(d_start_edge, start_edge, n_chunks * sizeof(u32))) return rc;
	if (int const rc = up(d_order, start_order, n_chunks * n_copies * sizeof(u32))) return rc;
	if (int const rc = up(d_div, start_divergence, n_chunks * n_copies * sizeof(u32))) return rc;
	size_t const pool_bytes(std::max<u64>(16, n_chunks * pool_capacity * sizeof(u32)));
	V2M_HIP_TRY(ctx, d_lhs.ensure(pool_bytes));
	V2M_HIP_TRY(ctx, d_rhs.ensure(pool_bytes));
	V2M_HIP_TRY(ctx, d_size.ensure(pool_bytes));
	V2M_HIP_TRY(ctx, d_end.ensure(n_cuts * sizeof(u64)));
	V2M_HIP_TRY(ctx, d_distinct.ensure(n_cuts * sizeof(u32)));
	V2M_HIP_TRY(ctx, d_first.ensure(n_cuts * sizeof(u32)));
	V2M_HIP_TRY(ctx, d_ref.ensure(n_cuts * sizeof(u32)));
	V2M_HIP_TRY(ctx, d_status.ensure(n_chunks * sizeof(u32)));
	V2M_HIP_TRY(ctx, hipMemsetAsync(d_status.p, 0xFF, n_chunks * sizeof(u32), ctx->stream));
	dev_buf d_class_scratch;                                  // the class arrays of the instantiations that do not hold them in LDS (more than 12 288 copies)
	hipError_t scratch_error(hipSuccess);
	auto const launch_records([&](auto per_tag) {
		constexpr int kPer(decltype(per_tag)::value);
		if (!v2m::kPbwtClassesInLds<kPer>) {
			scratch_error = d_class_scratch.ensure(size_t(n_chunks) * v2m::kPbwtClassScratchArrays * v2m::kPbwtThreads * kPer * sizeof(unsigned short));
			if (hipSuccess != scratch_error) return;
		}
		hipLaunchKernelGGL((v2m::pbwt_cut_records_kernel<kPer>), dim3(unsigned(n_chunks)), dim3(v2m::kPbwtThreads), 0, ctx->stream,
			d_by_edge, u32(cols / 64), u32(n_copies), u32(rows), d_cut_edge.as<u32>(), d_chunk_first.as<u64>(), d_start_edge.as<u32>(), d_order.as<u32>(), d_div.as<u32>(),
			pool_capacity, d_lhs.as<u32>(), d_rhs.as<u32>(), d_size.as<u32>(), d_end.as<u64>(), d_distinct.as<u32>(), d_first.as<u32>(), d_ref.as<u32>(), d_status.as<u32>(),
			d_class_scratch.as<unsigned short>());
	});
	pbwt_dispatch_per_thread<v2m::kPbwtPerThreadRecords>(ctx->path_cols, launch_records);
	V2M_HIP_TRY(ctx, scratch_error);
	V2M_HIP_TRY(ctx, hipGetLastError());
	V2M_HIP_TRY(ctx, hipMemcpyAsync(chunk_status, d_status.p, n_chunks * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
	u64 const cut_lo(chunk_first_cut[0]), cut_hi(chunk_first_cut[n_chunks]);   // only the cuts of this call's chunks
	if (cut_hi > cut_lo) {
		V2M_HIP_TRY(ctx, hipMemcpyAsync(rec_pool_end + cut_lo, d_end.as<u64>() + cut_lo, (cut_hi - cut_lo) * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(rec_distinct + cut_lo, d_distinct.as<u32>() + cut_lo, (cut_hi - cut_lo) * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(rec_first_class + cut_lo, d_first.as<u32>() + cut_lo, (cut_hi - cut_lo) * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(rec_first_is_ref + cut_lo, d_ref.as<u32>() + cut_lo, (cut_hi - cut_lo) * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
	}
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	for (u64 k(0); k < n_chunks; ++k) {
		if (0 != chunk_status[k]) { chunk_status[k] = 1; continue; }
		if (chunk_first_cut[k] == chunk_first_cut[k + 1]) continue;
		u64 const n(rec_pool_end[chunk_first_cut[k + 1] - 1]);
		if (n > pool_capacity) { chunk_status[k] = 1; continue; }
		V2M_HIP_TRY(ctx, hipMemcpyAsync(pool_lhs + k * pool_capacity, d_lhs.as<u32>() + k * pool_capacity, n * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(pool_rhs + k * pool_capacity, d_rhs.as<u32>() + k * pool_capacity, n * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(pool_size + k * pool_capacity, d_size.as<u32>() + k * pool_capacity, n * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
	}
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return V2M_OK;
}


// ---- rows -----------------------------------------------------------------------------------

int v2m_splice_rows_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_out, uint64_t row_pitch, uint64_t *row_lengths_out)
{
	if (int const rc = check_batch(ctx, rows, flags)) return rc;
	if (flags & V2M_SPLICE_BGZF) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "V2M_SPLICE_BGZF needs a sink (v2m_splice_rows): device rows are not compressed");
	if (0 == rows->n_rows) return V2M_OK;
	bool const unaligned(flags & V2M_SPLICE_UNALIGNED);
	if (!d_out || ((uintptr_t) d_out & 15)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_out must be a 16-byte aligned device pointer");
	u64 const need(unaligned ? v2m_max_unaligned_length(ctx) : ctx->view().length());
	if (row_pitch % 16 || row_pitch < ((need + 15) & ~u64(15)))
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "row_pitch must be a multiple of 16 and at least %llu rounded up to 16", (unsigned long long) need);
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!unaligned) {
		if (int const rc = splice_aligned_slice(ctx, rows, 0, rows->n_rows, static_cast<char *>(d_out), row_pitch)) return rc;
		if (row_lengths_out)
			for (u64 r(0); r < rows->n_rows; ++r) row_lengths_out[r] = ctx->view().length();
		return V2M_OK;
	}
	if (int const rc = splice_unaligned_slice(ctx, rows, 0, rows->n_rows, static_cast<char *>(d_out), row_pitch)) return rc;
	if (row_lengths_out) {
		V2M_HIP_TRY(ctx, hipMemcpyAsync(row_lengths_out, ctx->d_row_lengths.p, rows->n_rows * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	return V2M_OK;
}

int v2m_splice_rows(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_sink_fn sink, void *user)
{
	if (int const rc = check_batch(ctx, rows, flags)) return rc;
	if (!sink) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "sink is NULL");
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	bool const unaligned(flags & V2M_SPLICE_UNALIGNED);
	if ((flags & V2M_SPLICE_BGZF) && 0 != ctx->view().length()) return splice_rows_bgzf(ctx, rows, unaligned, sink, user);
	// a row is the sink's for the duration of its call only
	return splice_rows_pipeline(ctx, rows, unaligned, 2, "v2m_splice_rows", [&](v2m_row_hold &, slot_rows const &sl) -> int {
		for (u64 r(sl.r0); r < sl.r1; ++r)
			if (sink(user, r, sl.row(r), sl.bytes(r))) return fail(ctx, V2M_ERR_SINK, "sink aborted at row %llu", (unsigned long long) r);
		return V2M_OK;
	});
}


// ---- rows the sink may keep (ABI 5) -------------------------------------------------------------------------------------------
//
// v2m_splice_rows hands a row over for the duration of the sink call, so whatever the sink does with it -- a write() into a file --
// happens on the calling thread, one row at a time, and the next slice cannot be launched meanwhile: one context, one writer.
// Here a row stays where it is (a pinned slot of a ring of n_slots) until the sink says it is done with it, from any thread:
// the sink queues the row for a pool of writers and returns, the call goes on launching slices and copies, and only a slot whose
// rows are all released is copied into again.
int v2m_splice_rows_held(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, uint32_t n_slots, v2m_hold_sink_fn sink, void *user)
{
	if (int const rc = check_batch(ctx, rows, flags)) return rc;
	if (!sink) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "sink is NULL");
	if (flags & V2M_SPLICE_BGZF) return fail(ctx, V2M_ERR_UNSUPPORTED, "V2M_SPLICE_BGZF is not supported by v2m_splice_rows_held");
	if (n_slots < 2 || n_slots > 64) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "n_slots must be between 2 and 64 (got %u)", n_slots);
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	auto &state(ctx->held_state);
	// every row of the slice is held until released; when the sink refuses a row, that row and the rows after it count as never delivered
	return splice_rows_pipeline(ctx, rows, flags & V2M_SPLICE_UNALIGNED, n_slots, "v2m_splice_rows_held", [&](v2m_row_hold &slot, slot_rows const &sl) -> int {
		{ std::lock_guard<std::mutex> const lock(state.mutex); slot.outstanding = sl.r1 - sl.r0; }
		for (u64 r(sl.r0); r < sl.r1; ++r) {
			if (0 == sink(user, r, sl.row(r), sl.bytes(r), &slot)) continue;
			{ std::lock_guard<std::mutex> const lock(state.mutex); slot.outstanding -= sl.r1 - r; }   // (the only waiter is this thread)
			return fail(ctx, V2M_ERR_SINK, "sink aborted at row %llu", (unsigned long long) r);
		}
		return V2M_OK;
	});
}

void v2m_row_release(v2m_row_hold *hold)
{
	if (!hold) return;
	// Notified under the lock: the thread inside v2m_splice_rows_held returns once it sees the last slot at zero, and its caller may destroy
	// the ctx right after -- nothing of the ring is touched once the mutex is let go.
	std::lock_guard<std::mutex> const lock(hold->ring->mutex);
	if (hold->outstanding && 0 == --hold->outstanding) hold->ring->released.notify_all();
}



// ---- row alignment ops ------------------------------------------------------------------------------

namespace {

// The whole-row view for the duration of a call, whatever column window is in force; the window comes back untouched.
struct scoped_whole_rows {
	v2m_ctx *ctx;
	bool was;
	explicit scoped_whole_rows(v2m_ctx *c) : ctx(c), was(c->windowed) { c->windowed = false; }
	~scoped_whole_rows() { ctx->windowed = was; }
};

u64 ops_slice_budget()
{
	char const *const e(std::getenv("V2M_OPS_SLICE_BYTES"));   // test knob: small slices on small graphs
	return (e && *e) ? std::strtoull(e, nullptr, 10) : (u64(64) << 20);
}

// Passes 1 and 2 for rows [row_begin, row_end) of the batch over the whole view: effective edges, the unaligned tile offsets and row lengths
// (count_unaligned_kernel + scan_tile_counts_kernel, as the unaligned splice has them), breakpoints per row tile, op offsets and carried
// classes.  Leaves the rows' op counts (u32) and lengths (u64) in ctx->h_ops_stage, in that order, and returns their sum in *total_ops.
// split (V2M_OPS_SPLIT_MATCH): the _eqx kernels, timed under the same ids.
int row_ops_count_slice(v2m_ctx *ctx, v2m_row_batch const *rows, u64 row_begin, u64 row_end, bool split, u64 *total_ops)
{
	u64 const n_rows(row_end - row_begin);
	row_view &v(ctx->whole);
	if (int const rc = resolve_slice(ctx, rows, row_begin, row_end)) return rc;
	splice_grid g;
	if (int const rc = make_grid(ctx, n_rows, g)) return rc;
	u64 const cells(n_rows * v.n_tiles);
	V2M_HIP_TRY(ctx, ctx->d_row_lengths.ensure(n_rows * sizeof(u64)));
	V2M_HIP_TRY(ctx, ctx->d_tile_counts.ensure(cells * sizeof(u32)));
	V2M_HIP_TRY(ctx, ctx->d_ops_info.ensure(cells * sizeof(u32)));
	V2M_HIP_TRY(ctx, ctx->d_ops_offsets.ensure(cells * sizeof(u32)));
	V2M_HIP_TRY(ctx, ctx->d_ops_counts.ensure(n_rows * sizeof(u32)));
	v2m::tile_tables const tt{v.d_edge_begin.as<u32>(), v.d_cross_offsets.as<u32>(), v.d_cross_edges.as<u32>()};
	u64 const *const d_eff(ctx->d_eff.as<u64>() - v.words.restart);
	{
		u32 const count_rows(u32(std::min<u64>(n_rows, u64(v2m::kCountRowsMax))));
		u32 const count_groups(u32((n_rows + count_rows - 1) / count_rows));
		timed_launch tl(ctx, V2M_KERNEL_UNALIGNED_COUNT);
		hipLaunchKernelGGL(v2m::count_unaligned_kernel, dim3(unsigned(u64(v.n_tiles) * count_groups)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
			v.d_template0.as<v2m::vec4u>(), d_eff, v.words.stride, tt, ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
			ctx->d_tile_counts.as<u32>(), v.n_tiles, u32(n_rows), count_rows, count_groups, g.tile_run);
		hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(unsigned(n_rows)), dim3(256), 0, ctx->stream,
			ctx->d_tile_counts.as<u32>(), v.n_tiles, ctx->d_row_lengths.as<u64>());
	}
	{
		timed_launch tl(ctx, V2M_KERNEL_ROW_OPS_COUNT);
		hipLaunchKernelGGL(split ? v2m::count_row_ops_eqx_kernel : v2m::count_row_ops_kernel, dim3(unsigned(g.n_blocks)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
			v.d_template0.as<v2m::vec4u>(), d_eff, v.words.stride, tt, ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
			ctx->d_ops_info.as<u32>(), v.n_tiles, u32(n_rows), g.rows_per_group, g.n_groups, g.tile_run);
	}
	{
		timed_launch tl(ctx, V2M_KERNEL_ROW_OPS_SCAN);
		hipLaunchKernelGGL(split ? v2m::scan_row_ops_eqx_kernel : v2m::scan_row_ops_kernel, dim3(unsigned(n_rows)), dim3(256), 0, ctx->stream,
			ctx->d_ops_info.as<u32>(), ctx->d_ops_offsets.as<u32>(), v.n_tiles, ctx->d_ops_counts.as<u32>());
	}
	V2M_HIP_TRY(ctx, hipGetLastError());
	u64 const counts_bytes((n_rows * sizeof(u32) + 7) & ~u64(7));
	V2M_HIP_TRY(ctx, ctx->h_ops_stage.ensure(counts_bytes + 2 * n_rows * sizeof(u64)));
	V2M_POISON_HOST(ctx->h_ops_stage.p, counts_bytes + 2 * n_rows * sizeof(u64));
	char *const stage(ctx->h_ops_stage.as<char>());
	V2M_HIP_TRY(ctx, hipMemcpyAsync(stage, ctx->d_ops_counts.p, n_rows * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
	V2M_HIP_TRY(ctx, hipMemcpyAsync(stage + counts_bytes, ctx->d_row_lengths.p, n_rows * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	u32 const *const counts(reinterpret_cast<u32 const *>(stage));
	*total_ops = 0;
	for (u64 r(0); r < n_rows; ++r) *total_ops += counts[r];
	return V2M_OK;
}

// Pass 3 for rows [piece_begin, piece_end) of the slice of slice_rows rows that row_ops_count_slice has just counted (slice_begin = the slice's
// first row in the batch), and those rows to the sink.  The slice's tables are indexed by row, so a piece needs nothing counted again: it takes
// them from its first row on.
int row_ops_emit_piece(v2m_ctx *ctx, u64 slice_begin, u64 slice_rows, u64 piece_begin, u64 piece_end, bool split, v2m_ops_sink_fn sink, void *user)
{
	u64 const n_rows(piece_end - piece_begin);
	row_view &v(ctx->whole);
	u64 const counts_bytes((slice_rows * sizeof(u32) + 7) & ~u64(7));
	char *const stage(ctx->h_ops_stage.as<char>());
	u32 const *const counts(reinterpret_cast<u32 const *>(stage) + piece_begin);
	u64 const *const lengths(reinterpret_cast<u64 const *>(stage + counts_bytes) + piece_begin);
	u64 *const bases(reinterpret_cast<u64 *>(stage + counts_bytes + slice_rows * sizeof(u64)) + piece_begin);
	u64 total_ops(0);
	for (u64 r(0); r < n_rows; ++r) { bases[r] = total_ops; total_ops += counts[r]; }
	v2m::row_op_record const *records(nullptr);
	if (total_ops) {
		splice_grid g;
		if (int const rc = make_grid(ctx, n_rows, g)) return rc;
		V2M_HIP_TRY(ctx, ctx->d_ops_base.ensure(n_rows * sizeof(u64)));
		V2M_HIP_TRY(ctx, ctx->d_ops_out.ensure(total_ops * sizeof(v2m::row_op_record)));
		V2M_HIP_TRY(ctx, ctx->h_ops_out.ensure(total_ops * sizeof(v2m::row_op_record)));
		V2M_POISON_HOST(ctx->h_ops_out.p, total_ops * sizeof(v2m::row_op_record));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_ops_base.p, bases, n_rows * sizeof(u64), hipMemcpyHostToDevice, ctx->stream));
		v2m::tile_tables const tt{v.d_edge_begin.as<u32>(), v.d_cross_offsets.as<u32>(), v.d_cross_edges.as<u32>()};
		u64 const first_cell(piece_begin * v.n_tiles);
		{
			timed_launch tl(ctx, V2M_KERNEL_ROW_OPS_EMIT);
			hipLaunchKernelGGL(split ? v2m::emit_row_ops_eqx_kernel : v2m::emit_row_ops_kernel, dim3(unsigned(g.n_blocks)), dim3(v2m::kSpliceThreads), 0, ctx->stream,
				v.d_template0.as<v2m::vec4u>(), ctx->d_eff.as<u64>() - v.words.restart + piece_begin * v.words.stride, v.words.stride, tt, ctx->d_patches.as<v2m::edge_patch>(), ctx->d_labels.as<char>(),
				ctx->d_ops_info.as<u32>() + first_cell, v.n_tiles, u32(n_rows), g.rows_per_group, g.n_groups, g.tile_run,
				ctx->d_ops_offsets.as<u32>() + first_cell, ctx->d_ops_ref_before.as<u32>(), ctx->d_tile_counts.as<u32>() + first_cell, ctx->d_ops_base.as<u64>(),
				ctx->d_ops_out.as<v2m::row_op_record>(), total_ops);
		}
		V2M_HIP_TRY(ctx, hipGetLastError());
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->h_ops_out.p, ctx->d_ops_out.p, total_ops * sizeof(v2m::row_op_record), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		records = ctx->h_ops_out.as<v2m::row_op_record>();
	}
	// an op runs to the next breakpoint, the last one to the row's end (reference length, row length): in reference bytes for M (split: = and X)
	// and D, in row bytes for I.  Class 3 is M without the split and = with it; class 7 (X) comes from the _eqx kernels only.
	for (u64 r(0); r < n_rows; ++r) {
		u64 const n(counts[r]);
		ctx->ops_row.resize(n);
		for (u64 i(0); i < n; ++i) {
			v2m::row_op_record const &rec(records[bases[r] + i]);
			bool const last(i + 1 == n);
			u64 const next_ref(last ? ctx->ref_len : records[bases[r] + i + 1].ref_pos), next_row(last ? lengths[r] : records[bases[r] + i + 1].row_pos);
			bool const insertion(2 == rec.cls);
			ctx->ops_row[i].op = 3 == rec.cls ? (split ? V2M_OP_EQ : V2M_OP_M) : 7 == rec.cls ? V2M_OP_X : insertion ? V2M_OP_I : V2M_OP_D;
			ctx->ops_row[i].length = u32(insertion ? next_row - rec.row_pos : next_ref - rec.ref_pos);
		}
		u64 const row(slice_begin + piece_begin + r);
		if (sink(user, row, ctx->ops_row.data(), n, lengths[r]))
			return fail(ctx, V2M_ERR_SINK, "sink aborted at row %llu", (unsigned long long) row);
	}
	return V2M_OK;
}

} // namespace

int v2m_row_ops(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_ops_sink_fn sink, void *user)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (flags & ~V2M_OPS_SPLIT_MATCH) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "v2m_row_ops takes 0 or V2M_OPS_SPLIT_MATCH as flags (got 0x%x)", flags);
	bool const split(flags & V2M_OPS_SPLIT_MATCH);
	if (int const rc = check_batch(ctx, rows, V2M_SPLICE_UNALIGNED)) return rc;   // (the ops are read off the unaligned kernels' 0-padded rows: a NUL byte refuses as there)
	if (!sink) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "sink is NULL");
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	scoped_whole_rows const whole(ctx);
	row_view &v(ctx->whole);
	if (0 == ctx->aligned_len) {   // no column, no op
		for (u64 r(0); r < rows->n_rows; ++r)
			if (sink(user, r, nullptr, 0, 0)) return fail(ctx, V2M_ERR_SINK, "sink aborted at row %llu", (unsigned long long) r);
		return V2M_OK;
	}
	if (!v.has_template0) {
		if (int const rc = expand_reference(ctx, v, v.d_template0, 0)) return rc;
		v.has_template0 = true;
	}
	if (!ctx->has_ops_ref_before) {   // once per upload: the reference bytes before every tile
		scratch_buf total;
		V2M_HIP_TRY(ctx, ctx->d_ops_ref_before.ensure(std::max<size_t>(v.n_tiles * sizeof(u32), 16)));
		V2M_HIP_TRY(ctx, total.ensure(sizeof(u64)));
		hipLaunchKernelGGL(v2m::count_template_tiles_kernel, dim3(v.n_tiles), dim3(v2m::kSpliceThreads), 0, ctx->stream, v.d_template0.as<v2m::vec4u>(), ctx->d_ops_ref_before.as<u32>());
		hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->d_ops_ref_before.as<u32>(), v.n_tiles, total.as<u64>());
		V2M_HIP_TRY(ctx, hipGetLastError());
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		ctx->has_ops_ref_before = true;
	}

	// Slices: as many rows as keep what pass 1 and 2 leave per row -- three words per tile, and the effective-edge words (twice for rows with
	// cuts: their assembled bits) -- within 256 MiB.  A slice is counted once; what the scan says its rows' breakpoint records take then cuts it
	// into pieces of consecutive rows that fit the record budget (a single row goes through whatever it takes), each emitted from the slice's tables.
	u64 const budget_ops(std::max<u64>(1, ops_slice_budget() / sizeof(v2m::row_op_record)));
	u64 const row_bytes(12 * u64(v.n_tiles) + 16 * v.words.stride);
	u64 const want(std::max<u64>(1, std::min<u64>(rows->n_rows, (u64(256) << 20) / row_bytes)));
	for (u64 r0(0); r0 < rows->n_rows; r0 += want) {
		u64 const n(std::min<u64>(want, rows->n_rows - r0));
		u64 total_ops(0);
		if (int const rc = row_ops_count_slice(ctx, rows, r0, r0 + n, split, &total_ops)) return rc;
		u32 const *const counts(ctx->h_ops_stage.as<u32>());
		for (u64 p0(0); p0 < n;) {
			u64 p1(p0 + 1), piece_ops(counts[p0]);
			while (p1 < n && piece_ops + counts[p1] <= budget_ops) piece_ops += counts[p1++];
			if (int const rc = row_ops_emit_piece(ctx, r0, n, p0, p1, split, sink, user)) return rc;
			p0 = p1;
		}
	}
	return V2M_OK;
}


// ---- what the analyses share -----------------------------------------------------------------------
// The host-side steps that every analysis below (column counts to parsimony) takes the same way.  A new analysis starts from these.

extern "C++" {   // (templates and overloads, within the C ABI's block)
namespace {

// The stages of an analysis call, timed with events of their own while profiling is on (they have no V2M_KERNEL_* ids): a stage's
// segments are bracketed as they are queued and summed after the call's last synchronisation.  A segment is one event pair around
// everything the stage queues -- the counts and the pack segment span every slice -- so a figure is time elapsed on the stream, with
// whatever gaps the host's queueing leaves between the launches, not summed kernel time.
struct stage_times {
	enum { counts, pack, pairs, weights, weighted_pairs, n_stages };   // (the last two: the bootstrap's weighted path)
	struct segment { int stage; hipEvent_t begin, end; };
	v2m_ctx *ctx;
	std::vector<segment> segments;
	explicit stage_times(v2m_ctx *c) : ctx(c) {}
	stage_times(stage_times const &) = delete;
	~stage_times() { for (auto &s : segments) { (void) hipEventDestroy(s.begin); (void) hipEventDestroy(s.end); } }
	void begin(int stage)
	{
		if (!ctx->profiling) return;
		segment s{stage, nullptr, nullptr};
		if (hipSuccess != hipEventCreate(&s.begin)) return;
		if (hipSuccess != hipEventCreate(&s.end)) { (void) hipEventDestroy(s.begin); return; }
		(void) hipEventRecord(s.begin, ctx->stream);
		segments.push_back(s);
	}
	void end() { if (ctx->profiling && !segments.empty()) (void) hipEventRecord(segments.back().end, ctx->stream); }
	// a stage's sum, after the stream is idle
	double ms(int stage) const
	{
		double sum(0);
		for (auto const &s : segments) {
			float t(0);
			if (s.stage == stage && hipSuccess == hipEventElapsedTime(&t, s.begin, s.end)) sum += double(t);
		}
		return sum;
	}
};

// Takes `bytes` of a call's scratch; a refusal names the call (`prefix`), the size and the buffer (`what`).
int ensure_named(v2m_ctx *ctx, scratch_buf &buf, u64 bytes, char const *prefix, char const *what)
{
	hipError_t const st(buf.ensure(bytes));
	if (hipSuccess != st) return fail(ctx, hipErrorOutOfMemory == st ? V2M_ERR_OUT_OF_MEMORY : V2M_ERR_HIP, "%s: %llu bytes of %s: %s", prefix, (unsigned long long) bytes, what, hipGetErrorString(st));
	return V2M_OK;
}

// The same for pinned staging, which is host memory whatever the runtime calls its refusal.
int ensure_named(v2m_ctx *ctx, pinned_buf &buf, u64 bytes, char const *prefix, char const *what)
{
	if (hipSuccess != buf.ensure(bytes)) return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "%s: %llu bytes of pinned %s", prefix, (unsigned long long) bytes, what);
	return V2M_OK;
}

// The end of a call: leaves the compute stream, and the copy stream where the call used it, idle whatever happened.  Returns rc; the
// synchronisation's own error only when rc was V2M_OK.
int drain(v2m_ctx *ctx, int rc, bool both_streams)
{
	hipError_t const st(hipStreamSynchronize(ctx->stream));
	if (both_streams) (void) hipStreamSynchronize(ctx->copy_stream);
	if (V2M_OK == rc) V2M_HIP_TRY(ctx, st);
	return rc;
}

// Two buffers in turn: unit k is issued into device buffer and pinned slot k & 1 and crosses the link on the copy stream while unit
// k + 1 is issued; hand_over(k) waits for unit k's copy on the host, so both buffers of unit k are free again when unit k - 2 has been
// handed over, before unit k - 1 is queued.  Ends at the first status that is not V2M_OK and returns it.
template <typename t_issue, typename t_hand_over>
int in_turn(u64 n, t_issue const &issue, t_hand_over const &hand_over)
{
	for (u64 k(0); k < n; ++k) {
		if (int const rc = issue(k)) return rc;
		if (k >= 1) if (int const rc = hand_over(k - 1)) return rc;   // its copy ran under unit k's kernels
	}
	return n ? hand_over(n - 1) : V2M_OK;
}

// The tail of an issue: what the compute stream has queued so far into d_src crosses the link into pinned slot b, at host_offset.
// The caller records the slot's `copied` after the last copy of the unit.
int copy_to_slot(v2m_ctx *ctx, int b, void const *d_src, u64 bytes, u64 host_offset = 0)
{
	V2M_HIP_TRY(ctx, hipEventRecord(ctx->ev_compute[b], ctx->stream));
	V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute[b], 0));
	V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->host_slots[b]->host.as<char>() + host_offset, d_src, bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
	return V2M_OK;
}

int column_counts_zero(v2m_ctx *ctx, u32 *d_table, u64 plane_pitch, u64 L);
int column_counts_accumulate(v2m_ctx *ctx, v2m_row_batch const *rows, u32 *d_table, u64 plane_pitch);

// What the first half of a site selection leaves: the counts' table, the selection's blocks with their offsets, and the sites' number.
struct site_selection { u32 *table{}; u64 table_pitch{}; u32 *blocks{}; u64 select_blocks{}; u64 V{}; };

// The first half of a site selection, completed on the stream: the counts of the batch over the view in force into
// ctx->d_column_table, the rule's count kernel -- launch_count(table, table_pitch, blocks, select_blocks) -- over them, the scan of its
// blocks, and the total (d_column_total through h_column_total, whose second word is the caller's).  One segment of the counts stage;
// the caller's emit is the second.  n_rows >= 1, L >= 1.
template <typename t_launch>
int select_sites_count(v2m_ctx *ctx, v2m_row_batch const *rows, stage_times &times, char const *prefix, t_launch const &launch_count, site_selection &sel)
{
	u64 const L(ctx->view().length());
	sel.table_pitch = (L + 3) & ~u64(3);
	sel.select_blocks = (L + v2m::kSelectColumns - 1) / v2m::kSelectColumns;
	V2M_HIP_TRY(ctx, ctx->d_column_table.ensure(V2M_COUNT_CLASSES * sel.table_pitch * 4));
	V2M_HIP_TRY(ctx, ctx->d_column_blocks.ensure(std::max<u64>(sel.select_blocks * sizeof(u32), 16)));
	V2M_HIP_TRY(ctx, ctx->d_column_total.ensure(sizeof(u64)));
	V2M_HIP_TRY(ctx, ctx->h_column_total.ensure(2 * sizeof(u64)));
	V2M_POISON_HOST(ctx->h_column_total.p, 2 * sizeof(u64));
	sel.table = ctx->d_column_table.as<u32>();
	sel.blocks = ctx->d_column_blocks.as<u32>();
	times.begin(stage_times::counts);
	int rc(column_counts_zero(ctx, sel.table, sel.table_pitch, L));
	if (V2M_OK == rc) rc = column_counts_accumulate(ctx, rows, sel.table, sel.table_pitch);
	if (V2M_OK != rc) return rc;
	launch_count(sel.table, sel.table_pitch, sel.blocks, sel.select_blocks);
	hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(1), dim3(256), 0, ctx->stream, sel.blocks, u32(sel.select_blocks), ctx->d_column_total.as<u64>());
	times.end();
	if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "%s: the site selection did not launch", prefix);
	if (hipSuccess != hipMemcpyAsync(ctx->h_column_total.p, ctx->d_column_total.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream)
		|| hipSuccess != hipStreamSynchronize(ctx->stream))
		return fail(ctx, V2M_ERR_HIP, "%s: the site count did not arrive", prefix);
	sel.V = *ctx->h_column_total.as<u64>();
	if (sel.V > L) return fail(ctx, V2M_ERR_HIP, "the site selection counted %llu of %llu columns", (unsigned long long) sel.V, (unsigned long long) L);
	return V2M_OK;
}

// Both halves for the variable-site rule (snp: the SNP rule, site_kernels.hpp) over a batch of n rows.  The emit half takes `entries`
// >= sel.V >= 1 entries of `list` and leaves the sites' columns, relative to the view, in it; `emit_name` is what a refused launch is
// called.
int select_rule_sites_count(v2m_ctx *ctx, v2m_row_batch const *rows, bool snp, stage_times &times, char const *prefix, site_selection &sel)
{
	return select_sites_count(ctx, rows, times, prefix, [&](u32 *table, u64 table_pitch, u32 *blocks, u64 select_blocks) {
		if (snp)
			hipLaunchKernelGGL(v2m::count_snp_columns_kernel, dim3(unsigned(select_blocks)), dim3(v2m::kSelectColumns), 0, ctx->stream, table, table_pitch, ctx->view().length(), blocks);
		else
			hipLaunchKernelGGL(v2m::count_variable_columns_kernel, dim3(unsigned(select_blocks)), dim3(v2m::kSelectColumns), 0, ctx->stream,
				table, table_pitch, u64(0), ctx->view().length(), u32(rows->n_rows), 1u, blocks);
	}, sel);
}

int select_rule_sites_emit(v2m_ctx *ctx, u64 n, bool snp, stage_times &times, char const *prefix, site_selection const &sel, scratch_buf &list, u64 entries, char const *emit_name)
{
	u64 const L(ctx->view().length());
	if (int const rc = ensure_named(ctx, list, entries * sizeof(u32), prefix, "the site list")) return rc;
	u32 *const sites(list.as<u32>());
	times.begin(stage_times::counts);
	if (snp)
		hipLaunchKernelGGL(v2m::emit_snp_columns_kernel, dim3(unsigned(sel.select_blocks)), dim3(v2m::kSelectColumns), 0, ctx->stream, sel.table, sel.table_pitch, L, sel.blocks, sites, sel.V);
	else
		hipLaunchKernelGGL(v2m::emit_site_columns_kernel, dim3(unsigned(sel.select_blocks)), dim3(v2m::kSelectColumns), 0, ctx->stream,
			sel.table, sel.table_pitch, L, u32(n), sel.blocks, sites, sel.V);
	times.end();
	if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "%s: %s did not launch", prefix, emit_name);
	return V2M_OK;
}

// The V sites of ctx->d_site_columns through pinned staging to the host, completed: relative to the view, as the kernels leave them.
int fetch_site_columns(v2m_ctx *ctx, u64 V, char const *prefix, u32 const *&relative)
{
	if (int const rc = ensure_named(ctx, ctx->h_site_columns, V * sizeof(u32), prefix, "site list")) return rc;
	V2M_POISON_HOST(ctx->h_site_columns.p, V * sizeof(u32));
	if (hipSuccess != hipMemcpyAsync(ctx->h_site_columns.p, ctx->d_site_columns.p, V * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream)
		|| hipSuccess != hipStreamSynchronize(ctx->stream))
		return fail(ctx, V2M_ERR_HIP, "%s: the site list did not arrive", prefix);
	relative = ctx->h_site_columns.as<u32>();
	return V2M_OK;
}

} // namespace
} // extern "C++"


// ---- column counts ---------------------------------------------------------------------------------

namespace {

// What both column-count calls ask of their arguments, in check_batch's order; `allowed` is the call's one flag.
int check_column_counts(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, u32 allowed, char const *name)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows is NULL");
	if (flags & ~allowed) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s takes 0 or 0x%x as flags (got 0x%x): only the aligned form exists", name, allowed, flags);
	return check_batch(ctx, rows, 0);
}

// The rows of a launch of column_counts_kernel are spread over row groups so that a short view under many rows still fills the device: as many groups as
// bring the launch to about four workgroups per compute unit, of at least kColumnCountsMinRows rows and -- so that a group flushes its byte
// lanes once -- at most kCountRun.  V2M_COLUMN_COUNTS_ROWS_PER_GROUP overrides (a test knob, read per call: the kernel takes any value).
constexpr u64 kColumnCountsMinRows = 32;

u64 column_counts_rows_per_group(v2m_ctx const *ctx, u64 n_rows, u64 column_blocks)
{
	u64 const forced(env_u64("V2M_COLUMN_COUNTS_ROWS_PER_GROUP", 0));
	u64 const want_groups((4 * u64(ctx->n_cus) + column_blocks - 1) / column_blocks);
	u64 const spread(std::min<u64>(v2m::kCountRun, std::max<u64>(kColumnCountsMinRows, (n_rows + want_groups - 1) / want_groups)));
	return std::max<u64>({1, forced ? forced : spread, (n_rows + 65534) / 65535});   // (the grid's y)
}

// The kernels that walk a slice at its sites split its rows by the same rule (pack_sites_kernel and gather_sites_kernel: groups of at
// least 16 rows; ld_pack_kernel: of at least one 64-row word).  V2M_SITE_ROWS_PER_GROUP and V2M_SITE_LD_WORDS_PER_GROUP override it as
// V2M_COLUMN_COUNTS_ROWS_PER_GROUP does above, the floor included (test knobs, read once per call: the kernels take any value >= 1);
// the bound of the grid's y still holds.
u64 forced_site_group(u64 forced, u64 rule, u64 n)
{
	return forced ? std::max<u64>(forced, (n + 65534) / 65535) : rule;
}

// Adds the counts of the batch's rows over the view in force to the table: the batch in row slices through one device slot, per slice
// the aligned splice and column_counts_kernel.  Queues only; the caller synchronises.
// Staged form: when the call takes several slices and a full slice is one row group of at most kCountRun rows -- whole rows of a hundred
// million columns come five to a slice -- a slice would read and write 24 bytes of table per column for its few bytes of rows.  The
// kernel then carries its byte lanes from slice to slice in ctx->d_column_stage (6 bytes per column), and widen_column_counts_kernel
// adds them to the table before the rows since the last widening would exceed kCountRun, and after the last slice.
// V2M_COLUMN_COUNTS_STAGE=0 turns it off (measurement).
int column_counts_accumulate(v2m_ctx *ctx, v2m_row_batch const *rows, u32 *d_table, u64 plane_pitch)
{
	u64 const L(ctx->view().length());
	if (0 == L) return V2M_OK;
	slice_plan const p(plan_slices(ctx, rows->n_rows, false));
	u64 const column_blocks((L + v2m::kCountColumns - 1) / v2m::kCountColumns), chunks((L + 15) / 16);
	bool const staged(p.n_slices > 1 && p.rows_per_slice <= v2m::kCountRun && column_counts_rows_per_group(ctx, p.rows_per_slice, column_blocks) >= p.rows_per_slice
		&& 0 != env_u64("V2M_COLUMN_COUNTS_STAGE", 1));
	v2m::vec4u *d_stage(nullptr);
	if (staged) {
		V2M_HIP_TRY(ctx, ctx->d_column_stage.ensure(V2M_COUNT_CLASSES * chunks * 16));
		d_stage = ctx->d_column_stage.as<v2m::vec4u>();
		V2M_HIP_TRY(ctx, hipMemsetAsync(d_stage, 0, V2M_COUNT_CLASSES * chunks * 16, ctx->stream));
	}
	auto const widen([&] {
		hipLaunchKernelGGL(v2m::widen_column_counts_kernel, dim3(unsigned(column_blocks)), dim3(v2m::kCountThreads), 0, ctx->stream, d_stage, chunks, L, d_table, plane_pitch);
	});
	u64 staged_rows(0);
	for (u64 s(0); s < p.n_slices; ++s) {
		u64 const r0(s * p.rows_per_slice), r1(std::min(rows->n_rows, r0 + p.rows_per_slice)), nr(r1 - r0);
		V2M_HIP_TRY(ctx, ctx->ring[0].ensure(p.slot_bytes));   // (the slice takes its device slot: refilled in the checked build)
		char *const d_rows(ctx->ring[0].as<char>());
		if (int const rc = splice_aligned_slice(ctx, rows, r0, r1, d_rows, p.pitch)) return rc;
		u64 const per_group(staged ? nr : column_counts_rows_per_group(ctx, nr, column_blocks));
		u64 const groups((nr + per_group - 1) / per_group);
		{
			timed_launch tl(ctx, V2M_KERNEL_COLUMN_COUNTS);
			if (staged && staged_rows + nr > v2m::kCountRun) { widen(); staged_rows = 0; }
			hipLaunchKernelGGL(staged ? v2m::column_counts_kernel<true> : v2m::column_counts_kernel<false>, dim3(unsigned(column_blocks), unsigned(groups)), dim3(v2m::kCountThreads), 0, ctx->stream,
				d_rows, p.pitch, u32(nr), u32(std::min<u64>(per_group, nr)), L, d_table, plane_pitch, groups > 1 ? 1u : 0u, d_stage, chunks);
			staged_rows += nr;
			if (staged && s + 1 == p.n_slices) widen();
		}
		V2M_HIP_TRY(ctx, hipGetLastError());
	}
	return V2M_OK;
}

// Elements [0, (L + 3) & ~3) of every plane to 0.
int column_counts_zero(v2m_ctx *ctx, u32 *d_table, u64 plane_pitch, u64 L)
{
	if (0 == L) return V2M_OK;
	V2M_HIP_TRY(ctx, hipMemset2DAsync(d_table, plane_pitch * 4, 0, ((L + 3) & ~u64(3)) * 4, V2M_COUNT_CLASSES, ctx->stream));
	return V2M_OK;
}

} // namespace

int v2m_column_counts_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_counts, uint64_t plane_pitch)
{
	if (int const rc = check_column_counts(ctx, rows, flags, V2M_COUNTS_ACCUMULATE, "v2m_column_counts_device")) return rc;
	if (!d_counts) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_counts is NULL");
	if (reinterpret_cast<uintptr_t>(d_counts) & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_counts must be 16-byte aligned");
	u64 const L(ctx->view().length());
	if ((plane_pitch & 3) || plane_pitch < ((L + 3) & ~u64(3)))
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "plane_pitch %llu must be a multiple of 4 and at least %llu", (unsigned long long) plane_pitch, (unsigned long long) ((L + 3) & ~u64(3)));
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u32 *const table(static_cast<u32 *>(d_counts));
	int rc(V2M_OK);
	if (!(flags & V2M_COUNTS_ACCUMULATE)) rc = column_counts_zero(ctx, table, plane_pitch, L);
	if (V2M_OK == rc) rc = column_counts_accumulate(ctx, rows, table, plane_pitch);
	return drain(ctx, rc, false);
}

int v2m_column_counts(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_column_counts_sink_fn sink, void *user)
{
	if (int const rc = check_column_counts(ctx, rows, flags, V2M_COUNTS_VARIABLE_ONLY, "v2m_column_counts")) return rc;
	if (!sink) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "sink is NULL");
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const L(ctx->view().length()), view_begin(ctx->view().begin), n_rows(rows->n_rows);
	if (0 == L) return V2M_OK;
	u64 const pitch((L + 3) & ~u64(3));
	u32 const variable_only((flags & V2M_COUNTS_VARIABLE_ONLY) ? 1u : 0u);
	V2M_HIP_TRY(ctx, ctx->d_column_table.ensure(V2M_COUNT_CLASSES * pitch * 4));
	u32 *const table(ctx->d_column_table.as<u32>());
	if (int const rc = column_counts_zero(ctx, table, pitch, L)) return rc;

	// Column ranges whose records fit the block budget even when every column is selected; range k's records go to record buffer and
	// pinned slot k & 1, and the sink has range k - 1 while range k's kernels run.
	u64 const range_columns(std::max<u64>(1, std::min<u64>(L, env_u64("V2M_COLUMN_COUNTS_BLOCK_BYTES", u64(64) << 20) / sizeof(v2m_column_count))));
	u64 const n_ranges((L + range_columns - 1) / range_columns);
	u64 const range_blocks((range_columns + v2m::kSelectColumns - 1) / v2m::kSelectColumns);
	struct delivery { u64 n{}; bool pending{}; } deliveries[2];
	auto const deliver([&](delivery &d, v2m_row_hold &slot) -> int {
		if (!d.pending) return V2M_OK;
		d.pending = false;
		V2M_HIP_TRY(ctx, hipEventSynchronize(slot.copied));
		if (sink(user, slot.host.as<v2m_column_count>(), d.n)) return fail(ctx, V2M_ERR_SINK, "sink aborted");
		return V2M_OK;
	});
	auto const range([&](u64 k) -> int {
		u64 const c0(k * range_columns), c1(std::min(L, c0 + range_columns));
		u32 const blocks(u32((c1 - c0 + v2m::kSelectColumns - 1) / v2m::kSelectColumns));
		V2M_HIP_TRY(ctx, ctx->d_column_records[k & 1].ensure(range_columns * sizeof(v2m_column_count)));
		auto *const d_records(ctx->d_column_records[k & 1].as<v2m::column_count_record>());
		{
			timed_launch tl(ctx, V2M_KERNEL_COLUMN_SELECT);
			hipLaunchKernelGGL(v2m::count_variable_columns_kernel, dim3(blocks), dim3(v2m::kSelectColumns), 0, ctx->stream,
				table, pitch, c0, c1, u32(n_rows), variable_only, ctx->d_column_blocks.as<u32>());
			hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->d_column_blocks.as<u32>(), blocks, ctx->d_column_total.as<u64>());
			hipLaunchKernelGGL(v2m::emit_column_counts_kernel, dim3(blocks), dim3(v2m::kSelectColumns), 0, ctx->stream,
				table, pitch, c0, c1, view_begin, u32(n_rows), variable_only, ctx->d_column_blocks.as<u32>(), d_records, range_columns);
		}
		V2M_HIP_TRY(ctx, hipGetLastError());
		u64 *const h_total(ctx->h_column_total.as<u64>() + (k & 1));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(h_total, ctx->d_column_total.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
		if (k >= 1) if (int const rc = deliver(deliveries[(k - 1) & 1], *ctx->host_slots[(k - 1) & 1])) return rc;
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		u64 const n(*h_total);
		if (n > c1 - c0) return fail(ctx, V2M_ERR_HIP, "the column selection counted %llu of %llu columns", (unsigned long long) n, (unsigned long long) (c1 - c0));
		if (0 == n) return V2M_OK;
		v2m_row_hold &slot(*ctx->host_slots[k & 1]);
		V2M_HIP_TRY(ctx, slot.host.ensure(n * sizeof(v2m_column_count)));
		V2M_POISON_HOST(slot.host.p, n * sizeof(v2m_column_count));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(slot.host.p, d_records, n * sizeof(v2m_column_count), hipMemcpyDeviceToHost, ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipEventRecord(slot.copied, ctx->copy_stream));
		deliveries[k & 1].n = n;
		deliveries[k & 1].pending = true;
		return V2M_OK;
	});

	int rc(column_counts_accumulate(ctx, rows, table, pitch));
	if (V2M_OK == rc) rc = ensure_host_slots(ctx, 2, 0);
	if (V2M_OK == rc) {
		hipError_t st(ctx->d_column_blocks.ensure(std::max<u64>(range_blocks * sizeof(u32), 16)));
		if (hipSuccess == st) st = ctx->d_column_total.ensure(sizeof(u64));
		if (hipSuccess == st) st = ctx->h_column_total.ensure(2 * sizeof(u64));
		if (hipSuccess != st) rc = fail(ctx, hipErrorOutOfMemory == st ? V2M_ERR_OUT_OF_MEMORY : V2M_ERR_HIP, "column counts: %s", hipGetErrorString(st));
	}
	if (V2M_OK == rc) V2M_POISON_HOST(ctx->h_column_total.p, 2 * sizeof(u64));
	for (u64 k(0); k < n_ranges && V2M_OK == rc; ++k) rc = range(k);
	if (V2M_OK == rc) rc = deliver(deliveries[(n_ranges - 1) & 1], *ctx->host_slots[(n_ranges - 1) & 1]);
	// leave both streams idle whatever happened
	(void) hipStreamSynchronize(ctx->stream);
	(void) hipStreamSynchronize(ctx->copy_stream);
	return rc;
}


// ---- pair distances (distance_kernels.hpp) ---------------------------------------------------------

namespace {

int check_pair_distances(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, char const *name)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows is NULL");
	if (flags & ~u32(V2M_DIST_ACGT_ONLY)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s takes 0 or 0x%x as flags (got 0x%x)", name, V2M_DIST_ACGT_ONLY, flags);
	if (int const rc = check_batch(ctx, rows, 0)) return rc;
	if (rows->n_rows > V2M_PAIR_DISTANCES_MAX_ROWS)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes at most V2M_PAIR_DISTANCES_MAX_ROWS = %u rows (got %llu)", name, V2M_PAIR_DISTANCES_MAX_ROWS, (unsigned long long) rows->n_rows);
	if (ctx->view().length() >= (u64(1) << 32))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes a view of fewer than 2^32 columns (got %llu)", name, (unsigned long long) ctx->view().length());
	return V2M_OK;
}

// The parts the site chunks of a launch of pair_distances_kernel are split into: with few tile pairs, as many as bring the launch to
// about four workgroups per compute unit.  Returns the chunks of a part.  forced_parts: V2M_PAIR_DISTANCES_PARTS, which overrides the
// number of parts asked for (a test knob, read once per call: the kernel takes any split), or 0.
u64 pair_chunks_per_part(v2m_ctx const *ctx, u64 tile_pairs, u64 n_chunks, u64 forced)
{
	u64 const spread((4 * u64(ctx->n_cus) + tile_pairs - 1) / tile_pairs);
	u64 const want_parts(std::max<u64>(1, std::min<u64>({n_chunks, forced ? forced : spread, 65535})));
	return (n_chunks + want_parts - 1) / want_parts;
}

// What a call of pair_matrices_run computes: the plain matrix, weighted matrices (include/v2m_hip.h, "bootstrap"), or both.  The
// weighted matrices are made one after the other in d_weighted; after each is complete, with the stream idle, weighted_done(r) is
// called, and plain_done() after the plain one.  A callback that returns non-zero ends the call with that status.
struct pair_job {
	u32 *d_plain{}; u64 plain_pitch{};              // the plain matrix (pair_distances_kernel), or NULL
	u32 *d_weighted{}; u64 weighted_pitch{};        // one weighted matrix at a time
	u64 n_weighted{};                               // weighted matrices: 1 with explicit weights
	u32 const *weights{};                           // explicit weights, host, one per column of the view; or NULL: the draws of
	u64 seed{}; u32 first_replicate{};              //   replicates first_replicate, first_replicate + 1, ... (mod 2^32) under seed
	std::function<int()> plain_done;
	std::function<int(u64)> weighted_done;
	// what the call reports beside the info
	u64 n_pack_passes{}, max_slices{};
	double weights_ms{}, weighted_pairs_ms{};
};

// Queues and completes the call: the matrices of the batch over the view in force, u32[n_rows][pitch] each.  n_rows >= 1.
// Stage (1), the counts and the site list, runs once.  Then rounds: a round is every pass (the pack, then the pair kernels) for the
// plain matrix and the first weighted one together, or for one further weighted matrix.  Planes that fit the budget make one pass,
// which is packed in the first round only and stays resident.  info's three times are the plain path's; the job's are the weighted
// path's, the packs of later rounds among the weighted pairs.
int pair_matrices_run(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, pair_job &job, v2m_pair_distances_info *info)
{
	u64 const L(ctx->view().length()), n(rows->n_rows);
	stage_times times(ctx);
	v2m_pair_distances_info out{};
	out.n_columns = L;
	auto const zero_matrix([&](u32 *d, u64 pitch) -> int {
		V2M_HIP_TRY(ctx, hipMemset2DAsync(d, pitch * 4, 0, n * 4, n, ctx->stream));
		return V2M_OK;
	});
	auto const finish([&](int rc) -> int {
		if (V2M_OK == (rc = drain(ctx, rc, false))) {
			out.counts_ms = times.ms(stage_times::counts); out.pack_ms = times.ms(stage_times::pack); out.pairs_ms = times.ms(stage_times::pairs);
			job.weights_ms = times.ms(stage_times::weights); job.weighted_pairs_ms = times.ms(stage_times::weighted_pairs);
			if (info) *info = out;
		}
		return rc;
	});
	// no column, or no site: every matrix is zero
	auto const all_zero([&]() -> int {
		if (job.d_plain) {
			if (int const rc = zero_matrix(job.d_plain, job.plain_pitch)) return rc;
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			if (job.plain_done) if (int const rc = job.plain_done()) return rc;
		}
		for (u64 r(0); r < job.n_weighted; ++r) {
			if (int const rc = zero_matrix(job.d_weighted, job.weighted_pitch)) return rc;
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			if (job.weighted_done) if (int const rc = job.weighted_done(r)) return rc;
		}
		return V2M_OK;
	});
	if (0 == L) return finish(all_zero());

	// (1) the counts and the site list
	char const *const who("pair distances");
	site_selection sel;
	int rc(select_rule_sites_count(ctx, rows, false, times, who, sel));
	if (V2M_OK != rc) return finish(rc);
	u64 const V(sel.V);
	out.n_sites = V;
	if (0 == V) return finish(all_zero());
	if (V2M_OK != (rc = select_rule_sites_emit(ctx, n, false, times, who, sel, ctx->d_dist_sites, V, "emit_site_columns_kernel"))) return finish(rc);
	u32 *const sites(ctx->d_dist_sites.as<u32>());

	// the passes: ranges of whole chunks whose planes fit the budget
	u64 const n_tiles((n + v2m::kPairTile - 1) / v2m::kPairTile), n_pad(n_tiles * v2m::kPairTile), tile_pairs(n_tiles * (n_tiles + 1) / 2);
	u64 const chunk_sites(64 * u64(v2m::kPairChunkWords)), n_chunks((V + chunk_sites - 1) / chunk_sites);
	u64 const chunk_bytes(u64(v2m::kPairChunkWords) * 3 * n_pad * sizeof(u64));
	u64 const pass_chunks(std::max<u64>(1, std::min<u64>(n_chunks, env_u64("V2M_PAIR_DISTANCES_PLANE_BYTES", u64(16) << 30) / chunk_bytes)));
	u64 const n_passes((n_chunks + pass_chunks - 1) / pass_chunks);
	out.n_passes = n_passes;
	u64 const forced_parts(env_u64("V2M_PAIR_DISTANCES_PARTS", 0));
	u64 const forced_site_rows(env_u64("V2M_SITE_ROWS_PER_GROUP", 0));
	bool const atomics(n_passes > 1 || pair_chunks_per_part(ctx, tile_pairs, pass_chunks, forced_parts) < pass_chunks);
	bool const resident(1 == n_passes);
	slice_plan const p(plan_slices(ctx, n, false));

	// the weighted path's buffers, taken once a call
	u64 const n_words(n_chunks * v2m::kPairChunkWords);   // site words of the whole call, padding included: a slice
	u32 *w(nullptr), *any(nullptr), *h_any(nullptr);
	u64 *slices(nullptr);
	if (job.n_weighted) {
		if (V2M_OK != (rc = ensure_named(ctx, ctx->d_boot_weights, V * sizeof(u32), who, "site weights"))) return finish(rc);
		if (V2M_OK != (rc = ensure_named(ctx, ctx->d_boot_slices, u64(v2m::kBootSlices) * n_words * sizeof(u64), who, "weight slices"))) return finish(rc);
		if (V2M_OK != (rc = ensure_named(ctx, ctx->d_boot_any, 16, who, "the weights' OR"))) return finish(rc);
		w = ctx->d_boot_weights.as<u32>(); slices = ctx->d_boot_slices.as<u64>(); any = ctx->d_boot_any.as<u32>();
		h_any = reinterpret_cast<u32 *>(ctx->h_column_total.as<u64>() + 1);
		if (job.weights) {
			if (V2M_OK != (rc = ensure_named(ctx, ctx->d_boot_column_weights, L * sizeof(u32), who, "column weights"))) return finish(rc);
			if (hipSuccess != hipMemcpyAsync(ctx->d_boot_column_weights.p, job.weights, L * sizeof(u32), hipMemcpyHostToDevice, ctx->stream))
				return finish(fail(ctx, V2M_ERR_HIP, "pair distances: the weights could not be uploaded"));
		}
	}
	u64 const key(v2m::bootstrap_key(job.seed));

	// (2) the planes of a pass: zeroed (padding sites and rows hold code 0), then packed slice by slice
	auto const pack_pass([&](u64 chunks, u64 site_begin, u64 site_end) -> int {
		if (int const e = ensure_named(ctx, ctx->d_dist_planes, pass_chunks * chunk_bytes, who, "planes")) return e;   // (refilled per pack in the checked build)
		u64 *const planes(ctx->d_dist_planes.as<u64>());
		if (hipSuccess != hipMemsetAsync(planes, 0, chunks * chunk_bytes, ctx->stream)) return fail(ctx, V2M_ERR_HIP, "pair distances: the planes could not be zeroed");
		u64 const pack_blocks((site_end - site_begin + v2m::kPackThreads - 1) / v2m::kPackThreads);
		for (u64 s(0); s < p.n_slices; ++s) {
			u64 const r0(s * p.rows_per_slice), r1(std::min(n, r0 + p.rows_per_slice)), nr(r1 - r0);
			if (int const e = ensure_named(ctx, ctx->ring[0], p.slot_bytes, who, "the row slot")) return e;
			char *const d_rows(ctx->ring[0].as<char>());
			if (int const e = splice_aligned_slice(ctx, rows, r0, r1, d_rows, p.pitch)) return e;
			// row groups: with few site blocks, as many as bring the launch to about four workgroups per compute unit, of at least 16 rows
			u64 const want_groups((4 * u64(ctx->n_cus) + pack_blocks - 1) / pack_blocks);
			u64 const per_group(forced_site_group(forced_site_rows, std::max<u64>({16, (nr + want_groups - 1) / want_groups, (nr + 65534) / 65535}), nr));
			u64 const groups((nr + per_group - 1) / per_group);
			hipLaunchKernelGGL(v2m::pack_sites_kernel, dim3(unsigned(pack_blocks), unsigned(groups)), dim3(v2m::kPackThreads), 0, ctx->stream,
				d_rows, p.pitch, u32(nr), u32(per_group), u32(r0), sites, site_begin, site_end, planes, n_pad);
			if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "pair distances: pack_sites_kernel did not launch");
		}
		return V2M_OK;
	});

	// weighted matrix r's weights by site rank, their slices, and K: the one synchronisation that a matrix's weights cost
	auto const make_weights([&](u64 r, u32 &n_slices) -> int {
		times.begin(stage_times::weights);
		if (hipSuccess != hipMemsetAsync(any, 0, sizeof(u32), ctx->stream)) { times.end(); return fail(ctx, V2M_ERR_HIP, "bootstrap: the weights could not be zeroed"); }
		if (job.weights)
			hipLaunchKernelGGL(v2m::gather_site_weights_kernel, dim3(unsigned((V + v2m::kBootGatherThreads - 1) / v2m::kBootGatherThreads)), dim3(v2m::kBootGatherThreads), 0, ctx->stream,
				ctx->d_boot_column_weights.as<u32>(), sites, V, w);
		else {
			if (hipSuccess != hipMemsetAsync(w, 0, V * sizeof(u32), ctx->stream)) { times.end(); return fail(ctx, V2M_ERR_HIP, "bootstrap: the weights could not be zeroed"); }
			hipLaunchKernelGGL(v2m::bootstrap_weights_kernel, dim3(unsigned((L + v2m::kBootDrawThreads - 1) / v2m::kBootDrawThreads)), dim3(v2m::kBootDrawThreads), 0, ctx->stream,
				key, u32(job.first_replicate + u32(r)), L, sites, V, w);
		}
		hipLaunchKernelGGL(v2m::weight_slices_kernel, dim3(unsigned((n_words * 64 + v2m::kBootSliceThreads - 1) / v2m::kBootSliceThreads)), dim3(v2m::kBootSliceThreads), 0, ctx->stream,
			w, V, n_words, slices, any);
		times.end();
		if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "bootstrap: the weight kernels did not launch");
		if (hipSuccess != hipMemcpyAsync(h_any, any, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream) || hipSuccess != hipStreamSynchronize(ctx->stream))
			return fail(ctx, V2M_ERR_HIP, "bootstrap: the largest weight did not arrive");
		n_slices = 0;
		for (u32 bits(*h_any); bits; bits >>= 1) ++n_slices;
		job.max_slices = std::max<u64>(job.max_slices, n_slices);
		return V2M_OK;
	});

	bool packed(false);
	for (u64 round(0); 0 == round || round < job.n_weighted; ++round) {
		bool const plain(0 == round && job.d_plain), weighted(round < job.n_weighted);
		u32 n_slices(0);
		if (weighted && V2M_OK != (rc = make_weights(round, n_slices))) return finish(rc);
		if (plain && atomics) {
			times.begin(stage_times::pairs);
			rc = zero_matrix(job.d_plain, job.plain_pitch);
			times.end();
			if (V2M_OK != rc) return finish(rc);
		}
		if (weighted && (atomics || 0 == n_slices)) {
			times.begin(stage_times::weighted_pairs);
			rc = zero_matrix(job.d_weighted, job.weighted_pitch);
			times.end();
			if (V2M_OK != rc) return finish(rc);
		}
		bool const launches(plain || n_slices > 0);   // (K == 0: the zeros are the matrix, and nothing is launched)
		for (u64 pass(0); launches && pass < n_passes; ++pass) {
			u64 const c0(pass * pass_chunks), c1(std::min(n_chunks, c0 + pass_chunks)), chunks(c1 - c0);
			u64 const site_begin(c0 * chunk_sites), site_end(std::min(V, c1 * chunk_sites));
			if (!(resident && packed)) {
				times.begin(0 == round ? int(stage_times::pack) : int(stage_times::weighted_pairs));
				rc = pack_pass(chunks, site_begin, site_end);
				times.end();
				if (V2M_OK != rc) return finish(rc);
				packed = true;
				++job.n_pack_passes;
			}
			u64 const *const planes(ctx->d_dist_planes.as<u64>());
			// (3) the pairs
			u64 const per_part(pair_chunks_per_part(ctx, tile_pairs, chunks, forced_parts)), parts((chunks + per_part - 1) / per_part);
			if (plain) {
				times.begin(stage_times::pairs);
				hipLaunchKernelGGL((flags & V2M_DIST_ACGT_ONLY) ? v2m::pair_distances_kernel<true> : v2m::pair_distances_kernel<false>,
					dim3(unsigned(tile_pairs), 1, unsigned(parts)), dim3(v2m::kPairThreads), 0, ctx->stream,
					planes, n_pad, u32(chunks), u32(per_part), u32(n_tiles), u32(n), job.d_plain, job.plain_pitch, atomics ? 1u : 0u);
				times.end();
				if (hipSuccess != hipGetLastError()) return finish(fail(ctx, V2M_ERR_HIP, "pair distances: pair_distances_kernel did not launch"));
			}
			if (n_slices > 0) {
				times.begin(stage_times::weighted_pairs);
				hipLaunchKernelGGL((flags & V2M_DIST_ACGT_ONLY) ? v2m::pair_distances_weighted_kernel<true> : v2m::pair_distances_weighted_kernel<false>,
					dim3(unsigned(tile_pairs), 1, unsigned(parts)), dim3(v2m::kPairThreads), 0, ctx->stream,
					planes, n_pad, u32(chunks), u32(per_part), u32(n_tiles), u32(n), slices, n_words, c0 * v2m::kPairChunkWords, n_slices,
					job.d_weighted, job.weighted_pitch, atomics ? 1u : 0u);
				times.end();
				if (hipSuccess != hipGetLastError()) return finish(fail(ctx, V2M_ERR_HIP, "pair distances: pair_distances_weighted_kernel did not launch"));
			}
			if (pass + 1 < n_passes && hipSuccess != hipStreamSynchronize(ctx->stream))   // (the planes are reused, and refilled in the checked build)
				return finish(fail(ctx, V2M_ERR_HIP, "pair distances: pass %llu failed", (unsigned long long) pass));
		}
		if (plain && job.plain_done) {
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			if (V2M_OK != (rc = job.plain_done())) return finish(rc);
		}
		if (weighted && job.weighted_done) {
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			if (V2M_OK != (rc = job.weighted_done(round))) return finish(rc);
		}
	}
	return finish(V2M_OK);
}

// The plain matrix alone.
int pair_distances_run(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, u32 *d_dist, u64 pitch, v2m_pair_distances_info *info)
{
	pair_job job;
	job.d_plain = d_dist; job.plain_pitch = pitch;
	return pair_matrices_run(ctx, rows, flags, job, info);
}

} // namespace

int v2m_pair_distances_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_dist, uint64_t pitch)
{
	if (int const rc = check_pair_distances(ctx, rows, flags, "v2m_pair_distances_device")) return rc;
	if (!d_dist) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_dist is NULL");
	if (reinterpret_cast<uintptr_t>(d_dist) & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_dist must be 16-byte aligned");
	if ((pitch & 3) || pitch < rows->n_rows)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "pitch %llu must be a multiple of 4 and at least n_rows = %llu", (unsigned long long) pitch, (unsigned long long) rows->n_rows);
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	return pair_distances_run(ctx, rows, flags, static_cast<u32 *>(d_dist), pitch, nullptr);
}

int v2m_pair_distances(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, uint32_t *dist, v2m_pair_distances_info *info)
{
	if (int const rc = check_pair_distances(ctx, rows, flags, "v2m_pair_distances")) return rc;
	if (!dist) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dist is NULL");
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const n(rows->n_rows), pitch((n + 3) & ~u64(3));
	V2M_HIP_TRY(ctx, ctx->d_dist_matrix.ensure(n * pitch * 4));
	if (int const rc = pair_distances_run(ctx, rows, flags, ctx->d_dist_matrix.as<u32>(), pitch, info)) return rc;
	V2M_HIP_TRY(ctx, hipMemcpy2D(dist, n * 4, ctx->d_dist_matrix.p, pitch * 4, n * 4, n, hipMemcpyDeviceToHost));
	return V2M_OK;
}


// ---- variable sites (site_kernels.hpp) -------------------------------------------------------------

namespace {

int check_variable_sites(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, char const *name)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows is NULL");
	if (flags & ~u32(V2M_SITES_SNP)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s takes 0 or 0x%x as flags (got 0x%x)", name, V2M_SITES_SNP, flags);
	if (int const rc = check_batch(ctx, rows, 0)) return rc;
	if (ctx->view().length() >= (u64(1) << 32))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes a view of fewer than 2^32 columns (got %llu)", name, (unsigned long long) ctx->view().length());
	return V2M_OK;
}

// Stage (1): the counts of the batch over the view in force and the selection into ctx->d_site_columns (u32[V], readable up to
// (V + 3) & ~3 entries).  Completes on the stream; V to n_sites.  n_rows >= 1, L >= 1.
int variable_sites_select(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, stage_times &times, u64 &n_sites)
{
	bool const snp(flags & V2M_SITES_SNP);
	site_selection sel;
	if (int const rc = select_rule_sites_count(ctx, rows, snp, times, "variable sites", sel)) return rc;
	n_sites = sel.V;
	if (0 == sel.V) return V2M_OK;
	return select_rule_sites_emit(ctx, rows->n_rows, snp, times, "variable sites", sel, ctx->d_site_columns, (sel.V + 3) & ~u64(3), "the site list");
}

// Stage (2) for rows [r0, r1) of the batch: the aligned splice into ring slot 0, then gather_sites_kernel at the V sites of site_list
// (the context's list, or a 16-byte aligned range of it that ends with the list or at a multiple of four) into out, where batch row r
// lands at out + (r - out_first_row) * out_pitch.  forced_rows: V2M_SITE_ROWS_PER_GROUP as the call read it (0: the rule).  Queues only.
int variable_sites_gather_slice(v2m_ctx *ctx, v2m_row_batch const *rows, slice_plan const &p, u64 r0, u64 r1, u32 const *site_list, u64 V, char *out, u64 out_first_row, u64 out_pitch, u64 forced_rows, stage_times &times)
{
	u64 const nr(r1 - r0);
	if (int const rc = ensure_named(ctx, ctx->ring[0], p.slot_bytes, "variable sites", "the row slot")) return rc;   // (the slice takes its device slot: refilled in the checked build)
	char *const d_rows(ctx->ring[0].as<char>());
	times.begin(stage_times::pack);   // (the second pass's stage, as the pair distances number it)
	if (int const rc = splice_aligned_slice(ctx, rows, r0, r1, d_rows, p.pitch)) return rc;
	// row groups by pack_sites_kernel's rule: with few site blocks, as many as bring the launch to about four workgroups per compute
	// unit, of at least kGatherMinGroupRows rows
	u64 const block_sites(u64(v2m::kGatherThreads) * v2m::kGatherSites);
	u64 const site_blocks((V + block_sites - 1) / block_sites);
	u64 const want_groups((4 * u64(ctx->n_cus) + site_blocks - 1) / site_blocks);
	u64 const per_group(forced_site_group(forced_rows, std::max<u64>({u64(v2m::kGatherMinGroupRows), (nr + want_groups - 1) / want_groups, (nr + 65534) / 65535}), nr));
	u64 const groups((nr + per_group - 1) / per_group);
	hipLaunchKernelGGL(v2m::gather_sites_kernel, dim3(unsigned(site_blocks), unsigned(groups)), dim3(v2m::kGatherThreads), 0, ctx->stream,
		d_rows, p.pitch, u32(nr), u32(per_group), r0 - out_first_row, site_list, V, out, out_pitch);
	times.end();
	if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "variable sites: gather_sites_kernel did not launch");
	return V2M_OK;
}

} // namespace

int v2m_variable_sites_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_columns, void *d_bytes, uint64_t pitch, uint64_t *n_sites)
{
	if (int const rc = check_variable_sites(ctx, rows, flags, "v2m_variable_sites_device")) return rc;
	if (!d_bytes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_bytes is NULL");
	if (!n_sites) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "n_sites is NULL");
	if (reinterpret_cast<uintptr_t>(d_bytes) & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_bytes must be 16-byte aligned");
	if (reinterpret_cast<uintptr_t>(d_columns) & 3) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_columns must be 4-byte aligned");
	if (pitch & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "pitch %llu must be a multiple of 16", (unsigned long long) pitch);
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const L(ctx->view().length()), n(rows->n_rows);
	stage_times times(ctx);
	u64 V(0);
	int rc(0 == L ? V2M_OK : variable_sites_select(ctx, rows, flags, times, V));
	if (V2M_OK == rc) {
		*n_sites = V;
		if (V > pitch)
			rc = fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%llu sites do not fit a pitch of %llu: size the buffers for n_sites = %llu and call again",
				(unsigned long long) V, (unsigned long long) pitch, (unsigned long long) V);
	}
	if (V2M_OK == rc && V) {
		if (d_columns && hipSuccess != hipMemcpyAsync(d_columns, ctx->d_site_columns.p, V * sizeof(u32), hipMemcpyDeviceToDevice, ctx->stream))
			rc = fail(ctx, V2M_ERR_HIP, "variable sites: the site list could not be copied");
		slice_plan const p(plan_slices(ctx, n, false));
		u64 const forced_rows(env_u64("V2M_SITE_ROWS_PER_GROUP", 0));
		for (u64 s(0); s < p.n_slices && V2M_OK == rc; ++s)
			rc = variable_sites_gather_slice(ctx, rows, p, s * p.rows_per_slice, std::min(n, (s + 1) * p.rows_per_slice), ctx->d_site_columns.as<u32>(), V, static_cast<char *>(d_bytes), 0, pitch, forced_rows, times);
	}
	return drain(ctx, rc, false);
}

int v2m_variable_sites(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_site_columns_sink_fn columns_sink, v2m_site_rows_sink_fn rows_sink, void *user,
	v2m_variable_sites_info *info)
{
	if (int const rc = check_variable_sites(ctx, rows, flags, "v2m_variable_sites")) return rc;
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const L(ctx->view().length()), view_begin(ctx->view().begin), n(rows->n_rows);
	stage_times times(ctx);
	u64 V(0);
	auto const finish([&](int rc) -> int {
		if (V2M_OK == (rc = drain(ctx, rc, true)) && info) *info = v2m_variable_sites_info{V, L, times.ms(stage_times::counts), times.ms(stage_times::pack)};
		return rc;
	});
	if (0 == L) return finish(V2M_OK);
	if (int const rc = variable_sites_select(ctx, rows, flags, times, V)) return finish(rc);
	if (0 == V) return finish(V2M_OK);

	// the site list: over the link as it is, widened to absolute columns on the host
	if (columns_sink) {
		u32 const *relative(nullptr);
		if (int const rc = fetch_site_columns(ctx, V, "variable sites", relative)) return finish(rc);
		std::vector<u64> absolute(V);
		for (u64 i(0); i < V; ++i) absolute[i] = view_begin + relative[i];
		if (columns_sink(user, absolute.data(), V)) return finish(fail(ctx, V2M_ERR_SINK, "sink aborted"));
	}
	if (!rows_sink) return finish(V2M_OK);

	// Slice k is gathered into d_site_bytes[k & 1], crosses the link on the copy stream into pinned slot k & 1, and reaches the sink
	// while slice k + 1 is spliced and gathered.  Both buffers of slice k are free again when slice k - 2 has been handed over,
	// which waits for its copy on the host before slice k - 1 is queued.
	slice_plan const p(plan_slices(ctx, n, false));
	u64 const forced_rows(env_u64("V2M_SITE_ROWS_PER_GROUP", 0));
	u64 const out_pitch((V + 15) & ~u64(15)), slice_bytes(p.rows_per_slice * out_pitch);
	if (int const rc = ensure_host_slots(ctx, std::min<u64>(2, p.n_slices), slice_bytes)) return finish(rc);
	auto const first_row([&](u64 s) { return s * p.rows_per_slice; });
	auto const end_row([&](u64 s) { return std::min(n, (s + 1) * p.rows_per_slice); });
	auto const issue([&](u64 s) -> int {
		int const b(int(s & 1));
		v2m_row_hold &slot(*ctx->host_slots[b]);
		u64 const r0(first_row(s)), r1(end_row(s));
		if (int const rc = ensure_named(ctx, ctx->d_site_bytes[b], slice_bytes, "variable sites", "sites")) return rc;   // (refilled per slice in the checked build)
		V2M_POISON_HOST(slot.host.p, slice_bytes);
		if (int const rc = variable_sites_gather_slice(ctx, rows, p, r0, r1, ctx->d_site_columns.as<u32>(), V, ctx->d_site_bytes[b].as<char>(), r0, out_pitch, forced_rows, times)) return rc;
		if (int const rc = copy_to_slot(ctx, b, ctx->d_site_bytes[b].p, (r1 - r0) * out_pitch)) return rc;
		V2M_HIP_TRY(ctx, hipEventRecord(slot.copied, ctx->copy_stream));
		return V2M_OK;
	});
	auto const hand_over([&](u64 s) -> int {
		v2m_row_hold &slot(*ctx->host_slots[s & 1]);
		V2M_HIP_TRY(ctx, hipEventSynchronize(slot.copied));
		if (rows_sink(user, first_row(s), end_row(s) - first_row(s), slot.host.as<char>(), out_pitch, V)) return fail(ctx, V2M_ERR_SINK, "sink aborted");
		return V2M_OK;
	});
	return finish(in_turn(p.n_slices, issue, hand_over));
}


// ---- site LD (ld_kernels.hpp) ----------------------------------------------------------------------

namespace {

static_assert(sizeof(v2m_site_ld_params) == 24 && sizeof(v2m_ld_site) == 24 && sizeof(v2m_ld_pair) == 24 && sizeof(v2m_site_ld_info) == 56, "include/v2m_hip.h");
static_assert(sizeof(v2m_ld_site) == sizeof(v2m::ld_site_record) && sizeof(v2m_ld_pair) == sizeof(v2m::ld_pair_record), "the kernels' records");

int check_site_ld(v2m_ctx *ctx, v2m_row_batch const *rows, v2m_site_ld_params const *params, char const *name)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows is NULL");
	if (!params) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "params is NULL");
	if (params->window_sites < 1 || params->window_sites > V2M_SITE_LD_MAX_WINDOW)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s takes a window_sites of 1 to V2M_SITE_LD_MAX_WINDOW = %u (got %u)", name, V2M_SITE_LD_MAX_WINDOW, params->window_sites);
	if (params->min_allele_count < 1) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s takes a min_allele_count of at least 1 (got 0)", name);
	if (params->min_r2_den < 1 || params->min_r2_den > 1000000u || params->min_r2_num > params->min_r2_den)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s takes 1 <= min_r2_den <= 1000000 and min_r2_num <= min_r2_den (got %u / %u)", name, params->min_r2_num, params->min_r2_den);
	if (int const rc = check_batch(ctx, rows, 0)) return rc;
	if (rows->n_rows > V2M_SITE_LD_MAX_ROWS)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes at most V2M_SITE_LD_MAX_ROWS = %u rows (got %llu)", name, V2M_SITE_LD_MAX_ROWS, (unsigned long long) rows->n_rows);
	if (ctx->view().length() >= (u64(1) << 32))
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes a view of fewer than 2^32 columns (got %llu)", name, (unsigned long long) ctx->view().length());
	return V2M_OK;
}

// Where a call's results go: the device form's buffers, or the host form's sinks.
struct site_ld_dest {
	bool device;
	void *d_sites; u64 site_capacity; void *d_pairs; u64 pair_capacity; u64 *n_sites, *n_pairs;
	v2m_ld_sites_sink_fn sites_sink; v2m_ld_pairs_sink_fn pairs_sink; void *user; v2m_site_ld_info *info;
};

// The pairs (s, t), s < t < V, within both window limits: on the host, from the records' columns (ascending).
u64 site_ld_candidates(v2m_ld_site const *sites, u64 V, u64 window_sites, u64 window_columns)
{
	u64 total(0), reach(0);
	for (u64 s(0); s < V; ++s) {
		u64 last(std::min(V - 1, s + window_sites));
		if (window_columns) {
			if (reach < s) reach = s;
			while (reach + 1 < V && sites[reach + 1].column - sites[s].column <= window_columns) ++reach;
			last = std::min(last, reach);
		}
		total += last - s;
	}
	return total;
}

// Queues and completes the call.  n_rows >= 1.
int site_ld_run(v2m_ctx *ctx, v2m_row_batch const *rows, v2m_site_ld_params const &prm, site_ld_dest const &dest)
{
	u64 const L(ctx->view().length()), view_begin(ctx->view().begin), n(rows->n_rows);
	stage_times times(ctx);
	v2m_site_ld_info out{};
	out.n_columns = L;
	auto const finish([&](int rc) -> int {
		if (V2M_OK == (rc = drain(ctx, rc, true)) && dest.info) {
			out.counts_ms = times.ms(stage_times::counts); out.pack_ms = times.ms(stage_times::pack); out.pairs_ms = times.ms(stage_times::pairs);
			*dest.info = out;
		}
		return rc;
	});
	auto const nothing([&]() -> int {
		if (dest.device) { *dest.n_sites = 0; *dest.n_pairs = 0; }
		return finish(V2M_OK);
	});
	if (0 == L) return nothing();

	// (1) the counts and the number of sites
	char const *const who("site LD");
	site_selection sel;
	int rc(select_sites_count(ctx, rows, times, who, [&](u32 *table, u64 table_pitch, u32 *blocks, u64 select_blocks) {
		hipLaunchKernelGGL(v2m::count_ld_columns_kernel, dim3(unsigned(select_blocks)), dim3(v2m::kSelectColumns), 0, ctx->stream,
			table, table_pitch, L, prm.min_allele_count, blocks);
	}, sel));
	if (V2M_OK != rc) return finish(rc);
	u64 const V(sel.V);
	out.n_sites = V;
	if (0 == V) return nothing();

	u64 const n_strips((V + v2m::kLdTile - 1) / v2m::kLdTile), v_pad(n_strips * v2m::kLdTile), n_words((n + 63) / 64);
	u64 const plane_bytes(16 * v_pad * n_words), plane_budget(env_u64("V2M_SITE_LD_PLANE_BYTES", u64(16) << 30));
	if (plane_bytes > plane_budget)
		return finish(fail(ctx, V2M_ERR_UNSUPPORTED, "site LD: %llu sites of %llu rows need %llu bytes of planes, beyond V2M_SITE_LD_PLANE_BYTES = %llu",
			(unsigned long long) V, (unsigned long long) n, (unsigned long long) plane_bytes, (unsigned long long) plane_budget));
	u64 const n_blocks(std::min<u64>(n_strips, (u64(prm.window_sites) + v2m::kLdTile - 1) / v2m::kLdTile + 1));
	u64 const strip_cells(u64(v2m::kLdTile) * n_blocks);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->d_ld_sites, v_pad * sizeof(u32), who, "site list"))) return finish(rc);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->d_ld_records, V * sizeof(v2m_ld_site), who, "site records"))) return finish(rc);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->d_ld_planes, plane_bytes, who, "planes"))) return finish(rc);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->d_ld_cells, n_strips * strip_cells * sizeof(u32), who, "cells"))) return finish(rc);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->d_ld_totals, n_strips * sizeof(u64), who, "strip totals"))) return finish(rc);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->d_ld_bases, n_strips * sizeof(u64), who, "strip bases"))) return finish(rc);
	if (V2M_OK != (rc = ensure_named(ctx, ctx->h_ld_strips, 2 * n_strips * sizeof(u64), who, "strip totals"))) return finish(rc);
	V2M_POISON_HOST(ctx->h_ld_strips.p, 2 * n_strips * sizeof(u64));
	u32 *const sites(ctx->d_ld_sites.as<u32>());
	v2m::ld_site_record *const records(ctx->d_ld_records.as<v2m::ld_site_record>());
	u64 *const planes(ctx->d_ld_planes.as<u64>());
	u32 *const cells(ctx->d_ld_cells.as<u32>());
	u64 *const totals(ctx->d_ld_totals.as<u64>());
	u64 *const bases(ctx->d_ld_bases.as<u64>());
	times.begin(stage_times::counts);
	hipLaunchKernelGGL(v2m::emit_ld_columns_kernel, dim3(unsigned(sel.select_blocks)), dim3(v2m::kSelectColumns), 0, ctx->stream,
		sel.table, sel.table_pitch, L, prm.min_allele_count, view_begin, sel.blocks, sites, records, V);
	times.end();
	if (hipSuccess != hipGetLastError()) return finish(fail(ctx, V2M_ERR_HIP, "site LD: emit_ld_columns_kernel did not launch"));

	// (2) the planes: zeroed, then ORed into slice by slice
	slice_plan const p(plan_slices(ctx, n, false));
	u64 const forced_words(env_u64("V2M_SITE_LD_WORDS_PER_GROUP", 0));
	times.begin(stage_times::pack);
	if (hipSuccess != hipMemsetAsync(planes, 0, plane_bytes, ctx->stream)) return finish(fail(ctx, V2M_ERR_HIP, "site LD: the planes could not be zeroed"));
	u64 const pack_blocks((V + v2m::kLdPackThreads - 1) / v2m::kLdPackThreads);
	for (u64 s(0); s < p.n_slices; ++s) {
		u64 const r0(s * p.rows_per_slice), r1(std::min(n, r0 + p.rows_per_slice)), nr(r1 - r0);
		if (V2M_OK != (rc = ensure_named(ctx, ctx->ring[0], p.slot_bytes, who, "row slot"))) return finish(rc);
		char *const d_rows(ctx->ring[0].as<char>());
		if (V2M_OK != (rc = splice_aligned_slice(ctx, rows, r0, r1, d_rows, p.pitch))) return finish(rc);
		// word-aligned row groups: with few site blocks, as many as bring the launch to about four workgroups per compute unit
		u64 const words((r1 - 1) / 64 - r0 / 64 + 1);
		u64 const want_groups((4 * u64(ctx->n_cus) + pack_blocks - 1) / pack_blocks);
		u64 const per_group(forced_site_group(forced_words, std::max<u64>(1, (words + want_groups - 1) / want_groups), words));
		u64 const groups((words + per_group - 1) / per_group);
		hipLaunchKernelGGL(v2m::ld_pack_kernel, dim3(unsigned(pack_blocks), unsigned(groups)), dim3(v2m::kLdPackThreads), 0, ctx->stream,
			d_rows, p.pitch, u32(nr), u32(per_group), u32(r0), sites, records, V, planes, v_pad);
		if (hipSuccess != hipGetLastError()) return finish(fail(ctx, V2M_ERR_HIP, "site LD: ld_pack_kernel did not launch"));
	}
	times.end();

	// (3) the counts of the reported pairs per (site, tile), the offsets within every strip, the strips' totals
	auto const pairs_launch([&](bool emit, u64 strip_first, u64 strips, u64 out_base, void *d_out) {
		hipLaunchKernelGGL(emit ? v2m::ld_pairs_kernel<true> : v2m::ld_pairs_kernel<false>, dim3(unsigned(strips), unsigned(n_blocks)), dim3(v2m::kLdThreads), 0, ctx->stream,
			planes, v_pad, u32(n_words), sites, V, prm.window_sites, prm.window_columns, prm.min_r2_num, prm.min_r2_den,
			u32(strip_first), u32(n_strips), u32(n_blocks), cells, totals, bases, out_base, static_cast<v2m::ld_pair_record *>(d_out));
	});
	times.begin(stage_times::pairs);
	pairs_launch(false, 0, n_strips, 0, nullptr);
	hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(unsigned(n_strips)), dim3(256), 0, ctx->stream, cells, u32(strip_cells), totals);
	times.end();
	if (hipSuccess != hipGetLastError()) return finish(fail(ctx, V2M_ERR_HIP, "site LD: ld_pairs_kernel did not launch"));
	u64 *const h_totals(ctx->h_ld_strips.as<u64>()), *const h_bases(h_totals + n_strips);
	if (hipSuccess != hipMemcpyAsync(h_totals, totals, n_strips * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream)
		|| hipSuccess != hipStreamSynchronize(ctx->stream))
		return finish(fail(ctx, V2M_ERR_HIP, "site LD: the strip totals did not arrive"));
	u64 P(0);
	for (u64 i(0); i < n_strips; ++i) { h_bases[i] = P; P += h_totals[i]; }
	out.n_pairs = P;
	if (P && hipSuccess != hipMemcpyAsync(bases, h_bases, n_strips * sizeof(u64), hipMemcpyHostToDevice, ctx->stream))
		return finish(fail(ctx, V2M_ERR_HIP, "site LD: the strip bases could not be uploaded"));

	if (dest.device) {
		*dest.n_sites = V;
		*dest.n_pairs = P;
		if (V > dest.site_capacity || P > dest.pair_capacity)
			return finish(fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%llu sites and %llu pairs do not fit capacities of %llu and %llu: size the buffers for them and call again",
				(unsigned long long) V, (unsigned long long) P, (unsigned long long) dest.site_capacity, (unsigned long long) dest.pair_capacity));
		if (hipSuccess != hipMemcpyAsync(dest.d_sites, records, V * sizeof(v2m_ld_site), hipMemcpyDeviceToDevice, ctx->stream))
			return finish(fail(ctx, V2M_ERR_HIP, "site LD: the site records could not be copied"));
		if (P) {
			times.begin(stage_times::pairs);
			pairs_launch(true, 0, n_strips, 0, dest.d_pairs);
			times.end();
			if (hipSuccess != hipGetLastError()) return finish(fail(ctx, V2M_ERR_HIP, "site LD: ld_pairs_kernel did not launch"));
		}
		return finish(V2M_OK);
	}

	// the site records: over the link as they are
	if (dest.sites_sink || dest.info) {
		if (V2M_OK != (rc = ensure_named(ctx, ctx->h_ld_records, V * sizeof(v2m_ld_site), who, "site records"))) return finish(rc);
		V2M_POISON_HOST(ctx->h_ld_records.p, V * sizeof(v2m_ld_site));
		if (hipSuccess != hipMemcpyAsync(ctx->h_ld_records.p, records, V * sizeof(v2m_ld_site), hipMemcpyDeviceToHost, ctx->stream)
			|| hipSuccess != hipStreamSynchronize(ctx->stream))
			return finish(fail(ctx, V2M_ERR_HIP, "site LD: the site records did not arrive"));
		v2m_ld_site const *const h_sites(ctx->h_ld_records.as<v2m_ld_site>());
		out.n_candidates = site_ld_candidates(h_sites, V, prm.window_sites, prm.window_columns);
		if (dest.sites_sink && dest.sites_sink(dest.user, h_sites, V)) return finish(fail(ctx, V2M_ERR_SINK, "sink aborted"));
	}
	if (!dest.pairs_sink || 0 == P) return finish(V2M_OK);

	// The ranges: whole strips whose records fit the block, at least one strip; a range without a pair is passed over.  Range k is
	// emitted into d_ld_pairs[k & 1], crosses the link on the copy stream into pinned slot k & 1, and reaches the sink while range
	// k + 1 is emitted.  Both buffers of range k are free again when range k - 2 has been handed over, which waits for its copy on
	// the host before range k - 1 is queued.
	u64 const block_pairs(std::max<u64>(1, env_u64("V2M_SITE_LD_BLOCK_BYTES", u64(64) << 20) / sizeof(v2m_ld_pair)));
	struct range { u64 strip_begin, strip_end, base, pairs; };
	std::vector<range> ranges;
	u64 most(0);
	for (u64 i(0); i < n_strips;) {
		u64 j(i + 1), count(h_totals[i]);
		while (j < n_strips && count + h_totals[j] <= block_pairs) count += h_totals[j++];
		if (count) { ranges.push_back(range{i, j, h_bases[i], count}); most = std::max(most, count); }
		i = j;
	}
	if (int const rc2 = ensure_host_slots(ctx, std::min<u64>(2, ranges.size()), most * sizeof(v2m_ld_pair))) return finish(rc2);
	auto const issue([&](u64 k) -> int {
		int const b(int(k & 1));
		range const &g(ranges[k]);
		v2m_row_hold &slot(*ctx->host_slots[b]);
		if (int const rc2 = ensure_named(ctx, ctx->d_ld_pairs[b], most * sizeof(v2m_ld_pair), who, "pairs")) return rc2;   // (refilled per range in the checked build)
		V2M_POISON_HOST(slot.host.p, g.pairs * sizeof(v2m_ld_pair));
		times.begin(stage_times::pairs);
		pairs_launch(true, g.strip_begin, g.strip_end - g.strip_begin, g.base, ctx->d_ld_pairs[b].p);
		times.end();
		if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "site LD: ld_pairs_kernel did not launch");
		if (int const rc2 = copy_to_slot(ctx, b, ctx->d_ld_pairs[b].p, g.pairs * sizeof(v2m_ld_pair))) return rc2;
		V2M_HIP_TRY(ctx, hipEventRecord(slot.copied, ctx->copy_stream));
		return V2M_OK;
	});
	auto const hand_over([&](u64 k) -> int {
		v2m_row_hold &slot(*ctx->host_slots[k & 1]);
		V2M_HIP_TRY(ctx, hipEventSynchronize(slot.copied));
		if (dest.pairs_sink(dest.user, slot.host.as<v2m_ld_pair>(), ranges[k].pairs)) return fail(ctx, V2M_ERR_SINK, "sink aborted");
		return V2M_OK;
	});
	return finish(in_turn(ranges.size(), issue, hand_over));
}

} // namespace

int v2m_site_ld_device(v2m_ctx *ctx, const v2m_row_batch *rows, const v2m_site_ld_params *params, void *d_sites, uint64_t site_capacity, void *d_pairs, uint64_t pair_capacity,
	uint64_t *n_sites, uint64_t *n_pairs)
{
	if (int const rc = check_site_ld(ctx, rows, params, "v2m_site_ld_device")) return rc;
	if (!d_sites) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_sites is NULL");
	if (!d_pairs && pair_capacity) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_pairs is NULL with a pair_capacity of %llu", (unsigned long long) pair_capacity);
	if (!n_sites) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "n_sites is NULL");
	if (!n_pairs) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "n_pairs is NULL");
	if (reinterpret_cast<uintptr_t>(d_sites) & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_sites must be 16-byte aligned");
	if (reinterpret_cast<uintptr_t>(d_pairs) & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_pairs must be 16-byte aligned");
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	return site_ld_run(ctx, rows, *params, site_ld_dest{true, d_sites, site_capacity, d_pairs, pair_capacity, n_sites, n_pairs, nullptr, nullptr, nullptr, nullptr});
}

int v2m_site_ld(v2m_ctx *ctx, const v2m_row_batch *rows, const v2m_site_ld_params *params, v2m_ld_sites_sink_fn sites_sink, v2m_ld_pairs_sink_fn pairs_sink, void *user,
	v2m_site_ld_info *info)
{
	if (int const rc = check_site_ld(ctx, rows, params, "v2m_site_ld")) return rc;
	if (0 == rows->n_rows) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	return site_ld_run(ctx, rows, *params, site_ld_dest{false, nullptr, 0, nullptr, 0, nullptr, nullptr, sites_sink, pairs_sink, user, info});
}


// ---- neighbour joining (nj_kernels.hpp) ------------------------------------------------------------

namespace {

static_assert(sizeof(v2m_nj_node) == 40 && sizeof(v2m_nj_tree_info) == 48, "the header's sizes");
static_assert(V2M_NJ_NONE == v2m::kNjNone, "one value for no id");

int check_nj_matrix(v2m_ctx *ctx, void const *d_dist, u64 n, u64 pitch, v2m_nj_node const *nodes, char const *name)
{
	if (!d_dist) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_dist is NULL");
	if (!nodes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "nodes is NULL");
	if (reinterpret_cast<uintptr_t>(d_dist) & 15) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_dist must be 16-byte aligned");
	if ((pitch & 3) || pitch < n)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "pitch %llu must be a multiple of 4 and at least n = %llu", (unsigned long long) pitch, (unsigned long long) n);
	if (n > V2M_NJ_MAX_ROWS)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes at most V2M_NJ_MAX_ROWS = %u taxa (got %llu)", name, V2M_NJ_MAX_ROWS, (unsigned long long) n);
	return V2M_OK;
}

int nj_too_few(v2m_ctx *ctx, u64 n, char const *name)
{
	return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s needs at least 3 taxa: %llu %s no tree", name, (unsigned long long) n, 1 == n ? "has" : "have");
}

// Queues and completes the tree of the n >= 3 taxa of d_dist (u32[n][dist_pitch], device) into nodes (host, n - 2).  All launches go to
// the context's stream in order, none waits for the host; tree_ms: the stream time from the first to the last while profiling is on.
int nj_run(v2m_ctx *ctx, u32 const *d_dist, u64 n, u64 dist_pitch, v2m_nj_node *nodes, double *tree_ms)
{
	u64 const pitch((n + 1) & ~u64(1));
	char const *const who("neighbour joining");
	if (int const rc = ensure_named(ctx, ctx->d_nj_matrix, n * pitch * sizeof(double), who, "working matrix")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_nj_sums, pitch * sizeof(double), who, "row sums")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_nj_ids, pitch * sizeof(u32), who, "ids")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_nj_best, n * sizeof(v2m::nj_best), who, "row minima")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_nj_nodes, (n - 2) * sizeof(v2m_nj_node), who, "records")) return rc;
	double *const D(ctx->d_nj_matrix.as<double>()), *const R(ctx->d_nj_sums.as<double>());
	u32 *const ids(ctx->d_nj_ids.as<u32>());
	v2m::nj_best *const best(ctx->d_nj_best.as<v2m::nj_best>());
	v2m_nj_node *const d_nodes(ctx->d_nj_nodes.as<v2m_nj_node>());

	stage_times times(ctx);
	times.begin(0);
	hipLaunchKernelGGL(v2m::nj_init_kernel, dim3(unsigned(n)), dim3(v2m::kNjInitThreads), 0, ctx->stream, d_dist, dist_pitch, u32(n), D, pitch, R, ids);
	for (u64 t(0); t + 3 < n; ++t) {
		u32 const r(u32(n - t));
		unsigned const groups((r - 1 + v2m::kNjRowsPerGroup - 1) / v2m::kNjRowsPerGroup);
		hipLaunchKernelGGL(v2m::nj_rowmin_kernel, dim3(groups), dim3(v2m::kNjRowminThreads), 0, ctx->stream, D, pitch, R, ids, r, best);
		hipLaunchKernelGGL(v2m::nj_join_kernel, dim3(1), dim3(v2m::kNjJoinThreads), 0, ctx->stream, D, pitch, R, ids, r, u32(n + t), best, d_nodes + t);
	}
	hipLaunchKernelGGL(v2m::nj_last_kernel, dim3(1), dim3(v2m::kWave), 0, ctx->stream, D, pitch, ids, d_nodes + (n - 3));
	times.end();
	hipError_t const launched(hipGetLastError());
	hipError_t copied(hipMemcpyAsync(nodes, d_nodes, (n - 2) * sizeof(v2m_nj_node), hipMemcpyDeviceToHost, ctx->stream));
	hipError_t const st(hipStreamSynchronize(ctx->stream));   // (leave the stream idle whatever happened)
	if (hipSuccess != launched) return fail(ctx, V2M_ERR_HIP, "neighbour joining: a kernel did not launch: %s", hipGetErrorString(launched));
	V2M_HIP_TRY(ctx, copied);
	V2M_HIP_TRY(ctx, st);
	if (tree_ms) *tree_ms = times.ms(0);
	return V2M_OK;
}

} // namespace

int v2m_nj_tree_of_distances(v2m_ctx *ctx, const void *d_dist, uint64_t n, uint64_t pitch, v2m_nj_node *nodes, v2m_nj_tree_info *info)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (int const rc = check_nj_matrix(ctx, d_dist, n, pitch, nodes, "v2m_nj_tree_of_distances")) return rc;
	if (0 == n) return V2M_OK;
	if (n < 3) return nj_too_few(ctx, n, "v2m_nj_tree_of_distances");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	v2m_nj_tree_info out{};
	out.n_nodes = n - 2;
	if (int const rc = nj_run(ctx, static_cast<u32 const *>(d_dist), n, pitch, nodes, &out.tree_ms)) return rc;
	if (info) *info = out;
	return V2M_OK;
}

int v2m_nj_tree(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_nj_node *nodes, v2m_nj_tree_info *info)
{
	static_assert(V2M_NJ_MAX_ROWS == V2M_PAIR_DISTANCES_MAX_ROWS, "the pair distances' check bounds the taxa");
	if (int const rc = check_pair_distances(ctx, rows, flags, "v2m_nj_tree")) return rc;
	if (!nodes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "nodes is NULL");
	u64 const n(rows->n_rows), pitch((n + 3) & ~u64(3));
	if (0 == n) return V2M_OK;
	if (n < 3) return nj_too_few(ctx, n, "v2m_nj_tree");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	V2M_HIP_TRY(ctx, ctx->d_dist_matrix.ensure(n * pitch * 4));
	v2m_pair_distances_info distances{};
	if (int const rc = pair_distances_run(ctx, rows, flags, ctx->d_dist_matrix.as<u32>(), pitch, &distances)) return rc;
	v2m_nj_tree_info out{};
	out.n_nodes = n - 2;
	out.n_sites = distances.n_sites; out.n_columns = distances.n_columns; out.n_passes = distances.n_passes;
	out.distances_ms = distances.counts_ms + distances.pack_ms + distances.pairs_ms;
	if (int const rc = nj_run(ctx, ctx->d_dist_matrix.as<u32>(), n, pitch, nodes, &out.tree_ms)) return rc;
	if (info) *info = out;
	return V2M_OK;
}


// ---- bootstrap (bootstrap_kernels.hpp, nj_support.hpp) ---------------------------------------------

namespace {

static_assert(sizeof(v2m_nj_bootstrap_info) == 88, "the header's size");

// One weighted matrix through the context's matrix to the host: explicit weights, or replicate `replicate` under seed.
int weighted_distances_to_host(v2m_ctx *ctx, v2m_row_batch const *rows, u32 flags, u32 const *weights, u64 seed, u32 replicate, u32 *dist, v2m_pair_distances_info *info)
{
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const n(rows->n_rows), pitch((n + 3) & ~u64(3));
	V2M_HIP_TRY(ctx, ctx->d_boot_matrix.ensure(n * pitch * 4));
	pair_job job;
	job.d_weighted = ctx->d_boot_matrix.as<u32>(); job.weighted_pitch = pitch;
	job.n_weighted = 1; job.weights = weights; job.seed = seed; job.first_replicate = replicate;
	v2m_pair_distances_info out{};
	if (int const rc = pair_matrices_run(ctx, rows, flags, job, &out)) return rc;
	out.pairs_ms += job.weights_ms + job.weighted_pairs_ms;
	V2M_HIP_TRY(ctx, hipMemcpy2D(dist, n * 4, ctx->d_boot_matrix.p, pitch * 4, n * 4, n, hipMemcpyDeviceToHost));
	if (info) *info = out;
	return V2M_OK;
}

} // namespace

int v2m_pair_distances_weighted(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, const uint32_t *weights, uint32_t *dist, v2m_pair_distances_info *info)
{
	if (int const rc = check_pair_distances(ctx, rows, flags, "v2m_pair_distances_weighted")) return rc;
	if (!dist) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dist is NULL");
	u64 const L(ctx->view().length());
	if (!weights && L) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "weights is NULL");
	u64 sum(0);
	for (u64 c(0); c < L; ++c) sum += weights[c];   // (L < 2^32 values below 2^32: no overflow)
	if (sum >> 32) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "v2m_pair_distances_weighted takes weights that sum to less than 2^32 (got %llu)", (unsigned long long) sum);
	if (0 == rows->n_rows) return V2M_OK;
	return weighted_distances_to_host(ctx, rows, flags, weights, 0, 0, dist, info);
}

int v2m_bootstrap_distances(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, uint64_t seed, uint32_t replicate, uint32_t *dist, v2m_pair_distances_info *info)
{
	if (int const rc = check_pair_distances(ctx, rows, flags, "v2m_bootstrap_distances")) return rc;
	if (!dist) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dist is NULL");
	if (0 == rows->n_rows) return V2M_OK;
	return weighted_distances_to_host(ctx, rows, flags, nullptr, seed, replicate, dist, info);
}

int v2m_nj_bootstrap(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, uint32_t n_replicates, uint64_t seed, v2m_nj_node *nodes, uint32_t *support,
	v2m_nj_node *replicate_nodes, v2m_nj_bootstrap_info *info)
{
	if (int const rc = check_pair_distances(ctx, rows, flags, "v2m_nj_bootstrap")) return rc;
	if (!nodes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "nodes is NULL");
	if (0 == n_replicates || n_replicates > V2M_NJ_BOOTSTRAP_MAX_REPLICATES)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "v2m_nj_bootstrap takes 1 to V2M_NJ_BOOTSTRAP_MAX_REPLICATES = %u replicates (got %u)", V2M_NJ_BOOTSTRAP_MAX_REPLICATES, n_replicates);
	u64 const n(rows->n_rows), pitch((n + 3) & ~u64(3));
	if (0 == n) return V2M_OK;
	if (n < 3) return nj_too_few(ctx, n, "v2m_nj_bootstrap");
	if (!support && n > 3) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "support is NULL");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	V2M_HIP_TRY(ctx, ctx->d_dist_matrix.ensure(n * pitch * 4));
	V2M_HIP_TRY(ctx, ctx->d_boot_matrix.ensure(n * pitch * 4));
	v2m_nj_bootstrap_info out{};
	out.n_rows = n; out.n_replicates = n_replicates;
	try {
		v2m::nj_split_counter counter;
		std::vector<v2m_nj_node> tree(replicate_nodes ? 0 : n - 2);   // a replicate's records, where the caller keeps none
		pair_job job;
		job.d_plain = ctx->d_dist_matrix.as<u32>(); job.plain_pitch = pitch;
		job.d_weighted = ctx->d_boot_matrix.as<u32>(); job.weighted_pitch = pitch;
		job.n_weighted = n_replicates; job.seed = seed;
		job.plain_done = [&]() -> int {
			double ms(0);
			if (int const rc = nj_run(ctx, job.d_plain, n, pitch, nodes, &ms)) return rc;
			out.trees_ms += ms;
			std::string const err(counter.begin(n, nodes, support));
			return err.empty() ? V2M_OK : fail(ctx, V2M_ERR_HIP, "v2m_nj_bootstrap: the main tree: %s", err.c_str());
		};
		job.weighted_done = [&](u64 r) -> int {
			v2m_nj_node *const dst(replicate_nodes ? replicate_nodes + r * (n - 2) : tree.data());
			double ms(0);
			if (int const rc = nj_run(ctx, job.d_weighted, n, pitch, dst, &ms)) return rc;
			out.trees_ms += ms;
			std::string const err(counter.add(dst));
			return err.empty() ? V2M_OK : fail(ctx, V2M_ERR_HIP, "v2m_nj_bootstrap: replicate %llu: %s", (unsigned long long) r, err.c_str());
		};
		v2m_pair_distances_info distances{};
		if (int const rc = pair_matrices_run(ctx, rows, flags, job, &distances)) return rc;
		out.n_sites = distances.n_sites; out.n_columns = distances.n_columns; out.n_passes = distances.n_passes;
		out.n_pack_passes = job.n_pack_passes; out.max_slices = job.max_slices;
		out.distances_ms = distances.counts_ms + distances.pack_ms + distances.pairs_ms;
		out.weights_ms = job.weights_ms; out.pairs_ms = job.weighted_pairs_ms;
	} catch (std::bad_alloc const &) {
		(void) hipStreamSynchronize(ctx->stream);
		return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "v2m_nj_bootstrap: no host memory for the splits");
	}
	if (info) *info = out;
	return V2M_OK;
}


// ---- parsimony (parsimony_kernels.hpp) -------------------------------------------------------------

namespace {

static_assert(sizeof(v2m_parsimony_site) == 8 && sizeof(v2m_tree_site) == 16 && sizeof(v2m_tree_mutation) == 16 && sizeof(v2m_tree_parsimony_info) == 56, "the header's sizes");
static_assert(sizeof(v2m_parsimony_site) == sizeof(v2m::parsimony_site_record) && sizeof(v2m_tree_mutation) == sizeof(v2m::tree_mutation_record), "the kernels' records");

// What both forms refuse about the tree before any device work; 0 == n is the caller's.
int check_parsimony_tree(v2m_ctx *ctx, u64 n, v2m_nj_node const *nodes, char const *name)
{
	if (!nodes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "nodes is NULL");
	if (n < 3) return nj_too_few(ctx, n, name);
	if (n > V2M_NJ_MAX_ROWS)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes at most V2M_NJ_MAX_ROWS = %u taxa (got %llu)", name, V2M_NJ_MAX_ROWS, (unsigned long long) n);
	try {
		std::string err(v2m::nj_records_error(nodes, n));
		for (u64 t(0); err.empty() && t < n - 2; ++t) {
			if (nodes[t].a >= nodes[t].b || (t == n - 3 && nodes[t].b >= nodes[t].c))
				err = "record " + std::to_string(t) + " of the tree does not name its children in ascending order";
		}
		if (!err.empty()) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s: %s", name, err.c_str());
	} catch (std::bad_alloc const &) {
		return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "%s: no host memory for the tree's check", name);
	}
	return V2M_OK;
}

// The join table of a checked tree into ctx->d_fitch_joins (synchronous); the third child of the last record to last_c.
int parsimony_upload_tree(v2m_ctx *ctx, u64 n, v2m_nj_node const *nodes, u32 &last_c)
{
	try {
		std::vector<v2m::fitch_join> joins(n - 2);
		for (u64 t(0); t < n - 2; ++t) joins[t] = v2m::fitch_join{nodes[t].a, nodes[t].b};
		last_c = nodes[n - 3].c;
		V2M_HIP_TRY(ctx, ctx->d_fitch_joins.ensure(joins.size() * sizeof(v2m::fitch_join)));
		V2M_HIP_TRY(ctx, hipMemcpy(ctx->d_fitch_joins.p, joins.data(), joins.size() * sizeof(v2m::fitch_join), hipMemcpyHostToDevice));
	} catch (std::bad_alloc const &) {
		return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "parsimony: no host memory for the join table");
	}
	return V2M_OK;
}

u64 fitch_blocks(u64 V) { return (V + u64(v2m::kFitchThreads) * v2m::kFitchSites - 1) / (u64(v2m::kFitchThreads) * v2m::kFitchSites); }

// The scratch of one range of V >= 1 sites at `pitch`: the sets, the workgroups' steps, the total and its staging.
int parsimony_ensure(v2m_ctx *ctx, u64 n, u64 V, u64 pitch)
{
	if (int const rc = ensure_named(ctx, ctx->d_fitch_sets, (n - 2) * pitch, "parsimony", "sets")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_fitch_blocks, std::max<u64>(fitch_blocks(V) * sizeof(u32), 16), "parsimony", "workgroup steps")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_fitch_total, 2 * sizeof(u64), "parsimony", "totals")) return rc;
	V2M_HIP_TRY(ctx, ctx->h_fitch_total.ensure(sizeof(u64)));
	return V2M_OK;
}

// The up pass and the scan of one range, completed: the sets, d_sites[V], the workgroups' offsets, and the range's mutations to total.
int parsimony_up(v2m_ctx *ctx, unsigned char const *d_bytes, u64 n, u64 V, u64 pitch, u32 last_c, v2m::parsimony_site_record *d_sites, stage_times &times, u64 &total)
{
	unsigned const blocks(unsigned(fitch_blocks(V)));
	unsigned long long *const d_total(ctx->d_fitch_total.as<unsigned long long>());
	V2M_POISON_HOST(ctx->h_fitch_total.p, sizeof(u64));
	times.begin(stage_times::pairs);
	hipError_t st(hipMemsetAsync(d_total, 0, 2 * sizeof(u64), ctx->stream));
	hipLaunchKernelGGL(v2m::fitch_up_kernel, dim3(blocks), dim3(v2m::kFitchThreads), 0, ctx->stream,
		d_bytes, ctx->d_fitch_sets.as<unsigned char>(), pitch, u32(n), V, ctx->d_fitch_joins.as<v2m::fitch_join>(), last_c, d_sites, ctx->d_fitch_blocks.as<u32>(), d_total);
	hipLaunchKernelGGL(v2m::scan_tile_counts_kernel, dim3(1), dim3(256), 0, ctx->stream, ctx->d_fitch_blocks.as<u32>(), blocks, ctx->d_fitch_total.as<u64>() + 1);
	times.end();
	if (hipSuccess != st || hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "parsimony: the up pass did not launch");
	if (hipSuccess != hipMemcpyAsync(ctx->h_fitch_total.p, d_total, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream)
		|| hipSuccess != hipStreamSynchronize(ctx->stream))
		return fail(ctx, V2M_ERR_HIP, "parsimony: the number of mutations did not arrive");
	total = *ctx->h_fitch_total.as<u64>();
	return V2M_OK;
}

// Queues the down pass of the range the up pass left in the sets; d_mutations NULL: the branch counts only.
int parsimony_down(v2m_ctx *ctx, unsigned char const *d_bytes, u64 n, u64 V, u64 pitch, u32 last_c, v2m::parsimony_site_record const *d_sites, u32 *d_branches,
	u64 site_base, v2m::tree_mutation_record *d_mutations, stage_times &times)
{
	unsigned const blocks(unsigned(fitch_blocks(V)));
	times.begin(stage_times::pairs);
	hipLaunchKernelGGL(d_mutations ? v2m::fitch_down_kernel<true> : v2m::fitch_down_kernel<false>, dim3(blocks), dim3(v2m::kFitchThreads), 0, ctx->stream,
		d_bytes, ctx->d_fitch_sets.as<unsigned char>(), pitch, u32(n), V, ctx->d_fitch_joins.as<v2m::fitch_join>(), last_c, d_branches,
		d_sites, ctx->d_fitch_blocks.as<u32>(), u32(site_base), d_mutations);
	times.end();
	if (hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "parsimony: the down pass did not launch");
	return V2M_OK;
}

int parsimony_too_long(v2m_ctx *ctx, char const *name, u64 total)
{
	return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes a tree of fewer than 2^32 mutations (got %llu)", name, (unsigned long long) total);
}

} // namespace

int v2m_parsimony_of_sites(v2m_ctx *ctx, const void *d_bytes, uint64_t n, uint64_t n_sites, uint64_t pitch, const v2m_nj_node *nodes, void *d_sites, void *d_branch_changes,
	void *d_mutations, uint64_t capacity, uint64_t *n_mutations)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!n_mutations) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "n_mutations is NULL");
	if (0 == n) return V2M_OK;
	if (int const rc = check_parsimony_tree(ctx, n, nodes, "v2m_parsimony_of_sites")) return rc;
	u64 const V(n_sites);
	if (!d_bytes && V) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_bytes is NULL");
	if (!d_sites && V) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_sites is NULL");
	if (!d_branch_changes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_branch_changes is NULL");
	if (!d_mutations && capacity) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_mutations is NULL with a capacity of %llu", (unsigned long long) capacity);
	if ((reinterpret_cast<uintptr_t>(d_bytes) | reinterpret_cast<uintptr_t>(d_sites) | reinterpret_cast<uintptr_t>(d_branch_changes) | reinterpret_cast<uintptr_t>(d_mutations)) & 15)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_bytes, d_sites, d_branch_changes and d_mutations must be 16-byte aligned");
	if ((pitch & 15) || pitch < V)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "pitch %llu must be a multiple of 16 and at least n_sites = %llu", (unsigned long long) pitch, (unsigned long long) V);
	if (V >= (u64(1) << 32)) return fail(ctx, V2M_ERR_UNSUPPORTED, "v2m_parsimony_of_sites takes fewer than 2^32 sites (got %llu)", (unsigned long long) V);
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (0 == V) {
		*n_mutations = 0;
		V2M_HIP_TRY(ctx, hipMemsetAsync(d_branch_changes, 0, (2 * n - 3) * sizeof(u32), ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		return V2M_OK;
	}
	u32 last_c(0);
	if (int const rc = parsimony_upload_tree(ctx, n, nodes, last_c)) return rc;
	if (int const rc = parsimony_ensure(ctx, n, V, pitch)) return rc;
	stage_times times(ctx);
	u64 total(0);
	auto *const sites(static_cast<v2m::parsimony_site_record *>(d_sites));
	int rc(parsimony_up(ctx, static_cast<unsigned char const *>(d_bytes), n, V, pitch, last_c, sites, times, total));
	if (V2M_OK == rc) {
		*n_mutations = total;
		if (total >> 32) rc = parsimony_too_long(ctx, "v2m_parsimony_of_sites", total);
		else if (capacity && total > capacity)
			rc = fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%llu mutations do not fit a capacity of %llu: size d_mutations for n_mutations = %llu and call again",
				(unsigned long long) total, (unsigned long long) capacity, (unsigned long long) total);
	}
	if (V2M_OK == rc && hipSuccess != hipMemsetAsync(d_branch_changes, 0, (2 * n - 3) * sizeof(u32), ctx->stream)) rc = fail(ctx, V2M_ERR_HIP, "parsimony: the branch counts could not be zeroed");
	if (V2M_OK == rc)
		rc = parsimony_down(ctx, static_cast<unsigned char const *>(d_bytes), n, V, pitch, last_c, sites, static_cast<u32 *>(d_branch_changes), 0,
			capacity ? static_cast<v2m::tree_mutation_record *>(d_mutations) : nullptr, times);
	return drain(ctx, rc, false);
}

int v2m_tree_parsimony(v2m_ctx *ctx, const v2m_row_batch *rows, const v2m_nj_node *nodes, uint32_t flags, uint32_t *branch_changes, v2m_tree_sites_sink_fn sites_sink,
	v2m_tree_mutations_sink_fn mutations_sink, void *user, v2m_tree_parsimony_info *info)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows is NULL");
	if (flags) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "v2m_tree_parsimony takes 0 as flags (got 0x%x)", flags);
	if (int const rc = check_variable_sites(ctx, rows, V2M_SITES_SNP, "v2m_tree_parsimony")) return rc;
	u64 const n(rows->n_rows);
	if (0 == n) return V2M_OK;
	if (int const rc = check_parsimony_tree(ctx, n, nodes, "v2m_tree_parsimony")) return rc;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const L(ctx->view().length()), view_begin(ctx->view().begin), n_branches(2 * n - 3);
	stage_times times(ctx);
	u64 V(0), n_mutations(0), n_ranges(0);
	char const *const who("v2m_tree_parsimony");
	auto const finish([&](int rc) -> int {
		if (V2M_OK == (rc = drain(ctx, rc, true)) && info)
			*info = v2m_tree_parsimony_info{V, L, n_mutations, n_ranges, times.ms(stage_times::counts), times.ms(stage_times::pack), times.ms(stage_times::pairs)};
		return rc;
	});
	if (L) if (int const rc = variable_sites_select(ctx, rows, V2M_SITES_SNP, times, V)) return finish(rc);
	if (0 == V) {
		if (branch_changes) std::fill(branch_changes, branch_changes + n_branches, 0u);
		return finish(V2M_OK);
	}

	// Ranges of whole waves of sites whose leaf bytes and sets fit the budget.  Range k's records and mutations go to device buffers and
	// pinned slot k & 1 and cross the link on the copy stream while range k + 1 is gathered and walked; the mutations reach their sink
	// then, the records are kept for the one call of theirs after the last range.
	u64 const unit(u64(v2m::kFitchSites) * 64);
	u64 const budget_sites(env_u64("V2M_PARSIMONY_BYTES", u64(16) << 30) / (2 * n - 2));
	u64 const range_sites(std::min<u64>((V + unit - 1) / unit * unit, std::max<u64>(unit, budget_sites / unit * unit)));
	u64 const pitch((std::min(range_sites, V) + 15) & ~u64(15));
	n_ranges = (V + range_sites - 1) / range_sites;
	std::vector<v2m_tree_site> site_records;
	u32 last_c(0);
	try {
		if (sites_sink) site_records.resize(V);
	} catch (std::bad_alloc const &) {
		return finish(fail(ctx, V2M_ERR_OUT_OF_MEMORY, "v2m_tree_parsimony: no host memory for %llu site records", (unsigned long long) V));
	}
	if (sites_sink) {
		// the site list: over the link as it is, widened to absolute columns on the host
		u32 const *relative(nullptr);
		if (int const rc = fetch_site_columns(ctx, V, who, relative)) return finish(rc);
		for (u64 i(0); i < V; ++i) site_records[i].column = view_begin + relative[i];
	}
	if (int const rc = parsimony_upload_tree(ctx, n, nodes, last_c)) return finish(rc);
	if (int const rc = parsimony_ensure(ctx, n, std::min(range_sites, V), pitch)) return finish(rc);
	if (int const rc = ensure_host_slots(ctx, std::min<u64>(2, n_ranges), 0)) return finish(rc);
	{
		hipError_t st(ctx->d_fitch_bytes.ensure(n * pitch));
		if (hipSuccess == st) st = ctx->d_fitch_branches.ensure(n_branches * sizeof(u32));
		if (hipSuccess == st) st = hipMemsetAsync(ctx->d_fitch_branches.p, 0, n_branches * sizeof(u32), ctx->stream);
		if (hipSuccess != st) return finish(fail(ctx, hipErrorOutOfMemory == st ? V2M_ERR_OUT_OF_MEMORY : V2M_ERR_HIP, "v2m_tree_parsimony: %llu bytes of leaf rows: %s", (unsigned long long) (n * pitch), hipGetErrorString(st)));
	}
	unsigned char *const d_bytes(ctx->d_fitch_bytes.as<unsigned char>());
	slice_plan const p(plan_slices(ctx, n, false));
	u64 const gather_group_rows(env_u64("V2M_SITE_ROWS_PER_GROUP", 0));   // (the gather's test knob, read once per call)
	struct delivery { u64 first_site{}, n_sites{}, n_mutations{}, mutations_at{}; bool pending{}; } deliveries[2];
	auto const issue([&](u64 k) -> int {
		int const b(int(k & 1));
		u64 const s0(k * range_sites), Vr(std::min(V, s0 + range_sites) - s0);
		for (u64 s(0); s < p.n_slices; ++s)
			if (int const rc = variable_sites_gather_slice(ctx, rows, p, s * p.rows_per_slice, std::min(n, (s + 1) * p.rows_per_slice), ctx->d_site_columns.as<u32>() + s0, Vr,
				reinterpret_cast<char *>(d_bytes), 0, pitch, gather_group_rows, times)) return rc;
		if (int const rc = ensure_named(ctx, ctx->d_fitch_sites[b], Vr * sizeof(v2m_parsimony_site), who, "the site records")) return rc;
		auto *const d_sites(ctx->d_fitch_sites[b].as<v2m::parsimony_site_record>());
		u64 total(0);
		if (int const rc = parsimony_up(ctx, d_bytes, n, Vr, pitch, last_c, d_sites, times, total)) return rc;
		n_mutations += total;
		if (n_mutations >> 32) return parsimony_too_long(ctx, "v2m_tree_parsimony", n_mutations);
		bool const emit(mutations_sink && total);
		if (emit) if (int const rc = ensure_named(ctx, ctx->d_fitch_mutations[b], total * sizeof(v2m_tree_mutation), who, "mutations")) return rc;
		if (int const rc = parsimony_down(ctx, d_bytes, n, Vr, pitch, last_c, d_sites, ctx->d_fitch_branches.as<u32>(), s0,
			emit ? ctx->d_fitch_mutations[b].as<v2m::tree_mutation_record>() : nullptr, times)) return rc;
		delivery &d(deliveries[b]);
		d = delivery{s0, sites_sink ? Vr : 0, emit ? total : 0, (Vr * sizeof(v2m_parsimony_site) + 15) & ~u64(15), false};
		if (0 == d.n_sites && 0 == d.n_mutations) return V2M_OK;
		v2m_row_hold &slot(*ctx->host_slots[b]);
		u64 const slot_bytes(d.mutations_at + d.n_mutations * sizeof(v2m_tree_mutation));
		V2M_HIP_TRY(ctx, slot.host.ensure(slot_bytes));
		V2M_POISON_HOST(slot.host.p, slot_bytes);
		if (d.n_sites) if (int const rc = copy_to_slot(ctx, b, d_sites, Vr * sizeof(v2m_parsimony_site))) return rc;
		if (d.n_mutations) if (int const rc = copy_to_slot(ctx, b, ctx->d_fitch_mutations[b].p, d.n_mutations * sizeof(v2m_tree_mutation), d.mutations_at)) return rc;
		V2M_HIP_TRY(ctx, hipEventRecord(slot.copied, ctx->copy_stream));
		d.pending = true;
		return V2M_OK;
	});
	auto const hand_over([&](u64 k) -> int {
		delivery &d(deliveries[k & 1]);
		if (!d.pending) return V2M_OK;
		d.pending = false;
		v2m_row_hold &slot(*ctx->host_slots[k & 1]);
		V2M_HIP_TRY(ctx, hipEventSynchronize(slot.copied));
		auto const *const records(slot.host.as<v2m_parsimony_site>());
		for (u64 i(0); i < d.n_sites; ++i) {
			site_records[d.first_site + i].steps = records[i].steps;
			site_records[d.first_site + i].present = records[i].present;
		}
		if (d.n_mutations && mutations_sink(user, reinterpret_cast<v2m_tree_mutation const *>(slot.host.as<char>() + d.mutations_at), d.n_mutations))
			return fail(ctx, V2M_ERR_SINK, "sink aborted");
		return V2M_OK;
	});
	int rc(in_turn(n_ranges, issue, hand_over));
	if (V2M_OK == rc && branch_changes) {
		if (hipSuccess != hipMemcpyAsync(branch_changes, ctx->d_fitch_branches.p, n_branches * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream)
			|| hipSuccess != hipStreamSynchronize(ctx->stream))
			rc = fail(ctx, V2M_ERR_HIP, "v2m_tree_parsimony: the branch counts did not arrive");
	}
	if (V2M_OK == rc && sites_sink && sites_sink(user, site_records.data(), V)) rc = fail(ctx, V2M_ERR_SINK, "sink aborted");
	return finish(rc);
}


// ---- window diversity (diversity_kernels.hpp) ------------------------------------------------------

namespace {

static_assert(sizeof(v2m_diversity_bin) == 64 && sizeof(v2m_diversity_between_bin) == 32 && sizeof(v2m_window_diversity_info) == 40, "the header's sizes");
static_assert(sizeof(v2m_diversity_bin) == sizeof(v2m::diversity_bin_record) && sizeof(v2m_diversity_between_bin) == sizeof(v2m::diversity_between_record), "the kernels' records");
static_assert(V2M_DIVERSITY_MAX_ROWS == V2M_PAIR_DISTANCES_MAX_ROWS, "the limit of the pair distances");

// What both forms refuse about the bins and the sizes; `lo` and `hi` bound the columns a bin may hold (`what` names them).
int check_diversity_bins(v2m_ctx *ctx, u64 const *bounds, u64 n_bins, u64 lo, u64 hi, char const *what, u64 n_a, u64 n_b, u64 L, char const *name)
{
	if (!bounds) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bounds is NULL");
	for (u64 k(0); k < n_bins; ++k)
		if (bounds[k] > bounds[k + 1])
			return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s: bounds[%llu] = %llu descends to bounds[%llu] = %llu", name, (unsigned long long) k, (unsigned long long) bounds[k],
				(unsigned long long) (k + 1), (unsigned long long) bounds[k + 1]);
	if (n_bins && (bounds[0] < lo || bounds[n_bins] > hi))
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s: the bins [%llu, %llu) leave %s [%llu, %llu)", name, (unsigned long long) bounds[0], (unsigned long long) bounds[n_bins], what,
			(unsigned long long) lo, (unsigned long long) hi);
	if (std::max(n_a, n_b) > V2M_DIVERSITY_MAX_ROWS)
		return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes at most V2M_DIVERSITY_MAX_ROWS = %u rows a group (got %llu)", name, V2M_DIVERSITY_MAX_ROWS, (unsigned long long) std::max(n_a, n_b));
	if (L >= (u64(1) << 32)) return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes a view of fewer than 2^32 columns (got %llu)", name, (unsigned long long) L);
	if (n_bins >= 0xFFFFFFFFull) return fail(ctx, V2M_ERR_UNSUPPORTED, "%s takes fewer than 2^32 - 1 bins (got %llu)", name, (unsigned long long) n_bins);
	return V2M_OK;
}

// Queues the reduction of one table (table_b NULL) or two over the n_bins >= 1 bins of `bounds` (host, relative to the tables) into
// d_bins, and with d_sfs the spectrum of n_a / 2 + 1 entries; the count of multiallelic columns is left in ctx->d_diversity_multiallelic.
// The upload of the bounds is synchronous; nothing else waits for the host.
int diversity_run(v2m_ctx *ctx, u32 const *table_a, u32 const *table_b, u64 plane_pitch, u64 n_a, u64 n_b, u64 const *bounds, u64 n_bins, void *d_bins, void *d_sfs,
	stage_times &times)
{
	char const *const who("window diversity");
	if (int const rc = ensure_named(ctx, ctx->d_diversity_bounds, (n_bins + 1) * sizeof(u64), who, "bounds")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_diversity_multiallelic, 16, who, "the multiallelic count")) return rc;
	V2M_HIP_TRY(ctx, hipMemcpy(ctx->d_diversity_bounds.p, bounds, (n_bins + 1) * sizeof(u64), hipMemcpyHostToDevice));
	u64 const *const d_bounds(ctx->d_diversity_bounds.as<u64>());
	u64 const begin(bounds[0]), end(bounds[n_bins]);
	u32 const sfs_len(u32(n_a / 2 + 1));
	u32 const sfs_mode(!d_sfs ? 0u : sfs_len <= u32(v2m::kDiversitySfsLdsBins) ? 1u : 2u);
	times.begin(stage_times::pairs);
	hipError_t st(hipMemsetAsync(ctx->d_diversity_multiallelic.p, 0, 16, ctx->stream));
	if (hipSuccess == st && d_sfs) st = hipMemsetAsync(d_sfs, 0, u64(sfs_len) * sizeof(u64), ctx->stream);
	unsigned const init_blocks(unsigned((n_bins + 255) / 256));
	if (table_b) hipLaunchKernelGGL(v2m::diversity_init_kernel<true>, dim3(init_blocks), dim3(256), 0, ctx->stream, d_bounds, u32(n_bins), static_cast<u64 *>(d_bins));
	else hipLaunchKernelGGL(v2m::diversity_init_kernel<false>, dim3(init_blocks), dim3(256), 0, ctx->stream, d_bounds, u32(n_bins), static_cast<u64 *>(d_bins));
	if (begin < end) {
		u64 const first_tile(begin / v2m::kDiversityColumns), tiles((end - 1) / v2m::kDiversityColumns - first_tile + 1);
		hipLaunchKernelGGL(table_b ? v2m::diversity_bins_kernel<true> : v2m::diversity_bins_kernel<false>, dim3(unsigned(tiles)), dim3(v2m::kDiversityThreads), 0, ctx->stream,
			table_a, table_b, plane_pitch, d_bounds, u32(n_bins), u32(first_tile), u32(n_a), u32(n_b), static_cast<u64 *>(d_bins), static_cast<u64 *>(d_sfs),
			ctx->d_diversity_multiallelic.as<u64>(), sfs_mode);
	}
	times.end();
	if (hipSuccess != st || hipSuccess != hipGetLastError()) return fail(ctx, V2M_ERR_HIP, "window diversity: the reduction did not launch");
	return V2M_OK;
}

// The count the reduction left, to the host, completed.
int diversity_fetch_multiallelic(v2m_ctx *ctx, u64 &multiallelic)
{
	if (int const rc = ensure_named(ctx, ctx->h_diversity_multiallelic, sizeof(u64), "window diversity", "the multiallelic count")) return rc;
	V2M_POISON_HOST(ctx->h_diversity_multiallelic.p, sizeof(u64));
	if (hipSuccess != hipMemcpyAsync(ctx->h_diversity_multiallelic.p, ctx->d_diversity_multiallelic.p, sizeof(u64), hipMemcpyDeviceToHost, ctx->stream)
		|| hipSuccess != hipStreamSynchronize(ctx->stream))
		return fail(ctx, V2M_ERR_HIP, "window diversity: the multiallelic count did not arrive");
	multiallelic = *ctx->h_diversity_multiallelic.as<u64>();
	return V2M_OK;
}

} // namespace

int v2m_diversity_of_counts(v2m_ctx *ctx, const void *d_counts_a, const void *d_counts_b, uint64_t plane_pitch, uint64_t L, uint64_t n_a, uint64_t n_b,
	const uint64_t *bounds, uint64_t n_bins, void *d_bins, void *d_sfs, v2m_window_diversity_info *info)
{
	char const *const name("v2m_diversity_of_counts");
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!d_counts_a) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_counts_a is NULL");
	if (!d_bins) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_bins is NULL");
	if (!d_counts_b && n_b) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s: n_b = %llu without a second table", name, (unsigned long long) n_b);
	if (d_counts_b && d_sfs) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s: the between form has no spectrum: d_sfs must be NULL", name);
	if ((reinterpret_cast<uintptr_t>(d_counts_a) | reinterpret_cast<uintptr_t>(d_counts_b) | reinterpret_cast<uintptr_t>(d_bins) | reinterpret_cast<uintptr_t>(d_sfs)) & 15)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_counts_a, d_counts_b, d_bins and d_sfs must be 16-byte aligned");
	if ((plane_pitch & 3) || plane_pitch < ((L + 3) & ~u64(3)))
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "plane_pitch %llu must be a multiple of 4 and at least %llu", (unsigned long long) plane_pitch, (unsigned long long) ((L + 3) & ~u64(3)));
	if (int const rc = check_diversity_bins(ctx, bounds, n_bins, 0, L, "the table's columns", n_a, n_b, L, name)) return rc;
	if (0 == n_bins || 0 == n_a || (d_counts_b && 0 == n_b)) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	stage_times times(ctx);
	v2m_window_diversity_info out{};
	out.n_columns = L; out.n_bins = n_bins;
	int rc(diversity_run(ctx, static_cast<u32 const *>(d_counts_a), static_cast<u32 const *>(d_counts_b), plane_pitch, n_a, n_b, bounds, n_bins, d_bins, d_sfs, times));
	if (V2M_OK == rc) rc = diversity_fetch_multiallelic(ctx, out.multiallelic);
	if (V2M_OK == (rc = drain(ctx, rc, false)) && info) { out.bins_ms = times.ms(stage_times::pairs); *info = out; }
	return rc;
}

int v2m_window_diversity(v2m_ctx *ctx, const v2m_row_batch *rows_a, const v2m_row_batch *rows_b, const uint64_t *bounds, uint64_t n_bins, void *bins, uint64_t *sfs,
	v2m_window_diversity_info *info)
{
	char const *const name("v2m_window_diversity");
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!rows_a) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "rows_a is NULL");
	if (!bins) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bins is NULL");
	if (rows_b && sfs) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "%s: the between form has no spectrum: sfs must be NULL", name);
	if (int const rc = check_batch(ctx, rows_a, 0)) return rc;
	if (rows_b) if (int const rc = check_batch(ctx, rows_b, 0)) return rc;
	u64 const L(ctx->view().length()), view_begin(ctx->view().begin), n_a(rows_a->n_rows), n_b(rows_b ? rows_b->n_rows : 0);
	if (int const rc = check_diversity_bins(ctx, bounds, n_bins, view_begin, ctx->view().end, "the view", n_a, n_b, L, name)) return rc;
	if (0 == n_bins || 0 == n_a || (rows_b && 0 == n_b)) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	std::vector<u64> relative;
	try {
		relative.resize(n_bins + 1);
	} catch (std::bad_alloc const &) {
		return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "%s: no host memory for %llu bounds", name, (unsigned long long) (n_bins + 1));
	}
	for (u64 k(0); k <= n_bins; ++k) relative[k] = bounds[k] - view_begin;
	u64 const pitch((L + 3) & ~u64(3)), table_bytes(V2M_COUNT_CLASSES * pitch * 4), record_bytes(n_bins * (rows_b ? sizeof(v2m_diversity_between_bin) : sizeof(v2m_diversity_bin)));
	u64 const sfs_bytes((n_a / 2 + 1) * sizeof(u64));
	stage_times times(ctx);
	v2m_window_diversity_info out{};
	out.n_columns = L; out.n_bins = n_bins;
	auto const finish([&](int rc) -> int {
		if (V2M_OK == (rc = drain(ctx, rc, false)) && info) {
			out.counts_ms = times.ms(stage_times::counts); out.bins_ms = times.ms(stage_times::pairs);
			*info = out;
		}
		return rc;
	});
	V2M_HIP_TRY(ctx, ctx->d_column_table.ensure(table_bytes));
	if (rows_b) if (int const rc = ensure_named(ctx, ctx->d_diversity_table_b, table_bytes, name, "the second group's counts")) return rc;
	if (int const rc = ensure_named(ctx, ctx->d_diversity_records, record_bytes, name, "bin records")) return rc;
	if (sfs) if (int const rc = ensure_named(ctx, ctx->d_diversity_sfs, sfs_bytes, name, "the spectrum")) return rc;
	u32 *const table_a(ctx->d_column_table.as<u32>()), *const table_b(rows_b ? ctx->d_diversity_table_b.as<u32>() : nullptr);
	times.begin(stage_times::counts);
	int rc(column_counts_zero(ctx, table_a, pitch, L));
	if (V2M_OK == rc) rc = column_counts_accumulate(ctx, rows_a, table_a, pitch);
	if (V2M_OK == rc && rows_b) rc = column_counts_zero(ctx, table_b, pitch, L);
	if (V2M_OK == rc && rows_b) rc = column_counts_accumulate(ctx, rows_b, table_b, pitch);
	times.end();
	if (V2M_OK != rc) return finish(rc);
	if (V2M_OK != (rc = diversity_run(ctx, table_a, table_b, pitch, n_a, n_b, relative.data(), n_bins, ctx->d_diversity_records.p, sfs ? ctx->d_diversity_sfs.p : nullptr, times))) return finish(rc);
	if (hipSuccess != hipMemcpyAsync(bins, ctx->d_diversity_records.p, record_bytes, hipMemcpyDeviceToHost, ctx->stream)
		|| (sfs && hipSuccess != hipMemcpyAsync(sfs, ctx->d_diversity_sfs.p, sfs_bytes, hipMemcpyDeviceToHost, ctx->stream)))
		return finish(fail(ctx, V2M_ERR_HIP, "%s: the results did not leave the device", name));
	return finish(diversity_fetch_multiallelic(ctx, out.multiallelic));
}


// ---- output buffers ------------------------------------------------------------------------------

namespace {

// ms of the probe pattern on a buffer (best of two after a warm-up that populates the page tables)
int probe_output(v2m_ctx *ctx, void *p, u64 pitch, u32 n_groups, float &ms_out)
{
	scoped_events ev;
	V2M_HIP_TRY(ctx, ev.create(2));
	u32 const n_tiles(u32(pitch / v2m::kTileBytes));
	ms_out = 1e30f;
	for (int rep(0); rep < 3; ++rep) {
		V2M_HIP_TRY(ctx, hipEventRecord(ev[0], ctx->stream));
		hipLaunchKernelGGL(v2m::probe_write_kernel, dim3(n_tiles * n_groups), dim3(v2m::kSpliceThreads), 0, ctx->stream, static_cast<char *>(p), pitch, n_groups);
		V2M_HIP_TRY(ctx, hipEventRecord(ev[1], ctx->stream));
		V2M_HIP_TRY(ctx, hipEventSynchronize(ev[1]));
		float t(0);
		V2M_HIP_TRY(ctx, hipEventElapsedTime(&t, ev[0], ev[1]));
		if (rep) ms_out = std::min(ms_out, t);
	}
	return V2M_OK;
}

} // namespace

int v2m_alloc_output(v2m_ctx *ctx, uint64_t bytes, int candidates, void **d_out)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!d_out || 0 == bytes) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad v2m_alloc_output arguments");
	*d_out = nullptr;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	// the probe writes n_groups x 16 pseudo-rows of whole tiles; too small a buffer cannot be probed meaningfully
	u32 const n_groups(32);
	u64 const pitch((bytes / (n_groups * 16)) & ~u64(v2m::kTileBytes - 1));
	bool const can_probe(pitch >= u64(64) * v2m::kTileBytes);
	auto const note([&](std::string const &text) {
		if (ctx->info.size() > 2000) ctx->info.clear();   // keep the note bounded over many allocations
		if (!ctx->info.empty()) ctx->info += "; ";
		ctx->info += text;
	});

	// hipMalloc; with candidates > 1 several are held at once, the store pattern is timed on each and the fastest kept.
	// (Buffers mapped from physically contiguous chunks with hipMemCreate / hipMemMap write at the same rate as the best
	// hipMalloc'ed ones, but that API is not used: on this stack (ROCm 7.2) a range that is unmapped, freed and mapped again
	// keeps stale address translations -- rows written into a re-mapped buffer were silently lost, and the round-1 probe's
	// GPU memory access fault was the same thing -- see profiles/r02/output_buffer_vmm_reuse.txt.)
	struct candidate_set {
		std::vector<void *> bufs;
		void *keep{};
		~candidate_set() { for (void *p : bufs) if (p != keep) (void) hipFree(p); }
	} cs;
	bool const probe(candidates > 1 && can_probe);
	for (int c(0); c < (probe ? candidates : 1); ++c) {
		void *p(nullptr);
		hipError_t const st(hipMalloc(&p, bytes));
		if (hipSuccess != st) {
			(void) hipGetLastError();
			if (cs.bufs.empty()) return fail(ctx, V2M_ERR_OUT_OF_MEMORY, "hipMalloc of %llu bytes failed: %s", (unsigned long long) bytes, hipGetErrorString(st));
			break;   // keep what fits
		}
		cs.bufs.push_back(p);
	}
	std::size_t best(0);
	if (probe && cs.bufs.size() > 1) {
		std::vector<float> ms;
		for (void *p : cs.bufs) {
			float t(0);
			if (int const rc = probe_output(ctx, p, pitch, n_groups, t)) return rc;   // cs frees every candidate
			ms.push_back(t);
		}
		best = std::size_t(std::min_element(ms.begin(), ms.end()) - ms.begin());
		std::string text("output buffer chosen among " + std::to_string(cs.bufs.size()) + " hipMalloc candidates by probe write rate (GB/s):");
		for (float const t : ms) { char b2[32]; std::snprintf(b2, sizeof(b2), " %.0f", double(pitch) * n_groups * 16 / (t * 1e6)); text += b2; }
		note(text);
	}
	cs.keep = cs.bufs[best];
	*d_out = cs.keep;
	return V2M_OK;
}

int v2m_free_output(v2m_ctx *ctx, void *d_ptr)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (!d_ptr) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	V2M_HIP_TRY(ctx, hipFree(d_ptr));
	return V2M_OK;
}

int v2m_read_output(v2m_ctx *ctx, const void *d_src, uint64_t bytes, void *dst)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (0 == bytes) return V2M_OK;
	if (!d_src) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "d_src is NULL");
	if (!dst) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dst is NULL");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	V2M_HIP_TRY(ctx, hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
	return V2M_OK;
}



// ---- BGZF ------------------------------------------------------------------------------------------

uint64_t v2m_bgzf_bound(uint64_t n)
{
	return 0 == n ? 28 : n + v2m::kBgzfStoredOverhead * bgzf_pieces(n);
}

int v2m_bgzf_frame_stored(const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out)
{
	static unsigned char const eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	if ((n && !src) || !n_out || (!dst && cap)) return V2M_ERR_INVALID_ARGUMENT;
	*n_out = 0;
	u64 const need(v2m_bgzf_bound(n));
	if (cap < need) return V2M_ERR_INVALID_ARGUMENT;
	unsigned char *out(static_cast<unsigned char *>(dst));
	if (0 == n) { std::memcpy(out, eof, sizeof(eof)); *n_out = sizeof(eof); return V2M_OK; }
	unsigned char const *in(static_cast<unsigned char const *>(src));
	auto const le16([](unsigned char *p, u32 v) { p[0] = v & 255; p[1] = (v >> 8) & 255; });
	auto const le32([&](unsigned char *p, u32 v) { le16(p, v); le16(p + 2, v >> 16); });
	for (u64 done(0); done < n;) {
		u32 const piece(u32(std::min<u64>(n - done, v2m::kBgzfBlockBytes)));
		std::memcpy(out, eof, 16);                                   // the header up to BSIZE
		le16(out + 16, piece + v2m::kBgzfStoredOverhead - 1);
		out[18] = 1;                                                 // BFINAL, BTYPE 00
		le16(out + 19, piece);
		le16(out + 21, ~piece & 0xffffu);
		std::memcpy(out + 23, in + done, piece);
		le32(out + 23 + piece, crc32_host(in + done, piece));
		le32(out + 27 + piece, piece);
		out += piece + v2m::kBgzfStoredOverhead;
		done += piece;
	}
	*n_out = need;
	return V2M_OK;
}

int v2m_bgzf_compress(v2m_ctx *ctx, const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if ((n && !src) || !n_out) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "src or n_out is NULL");
	*n_out = 0;
	if (0 == n) return V2M_OK;
	if (!dst) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dst is NULL");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	u64 const chunk_max(u64(v2m::kBgzfBlockBytes) * 4096);   // 267 MB of input per pass
	u64 const first(std::min(n, chunk_max));
	V2M_HIP_TRY(ctx, ctx->d_bgzf_in.ensure((first + 15) & ~u64(15)));
	V2M_HIP_TRY(ctx, ctx->d_bgzf_dense[0].ensure(v2m_bgzf_bound(first)));
	u64 written(0);
	for (u64 done(0); done < n;) {
		u64 const chunk(std::min(n - done, chunk_max));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bgzf_in.p, static_cast<char const *>(src) + done, chunk, hipMemcpyHostToDevice, ctx->stream));
		if (int const rc = bgzf_encode_rows(ctx, ctx->d_bgzf_in.as<char>(), 0, nullptr, chunk, chunk, 1, ctx->d_bgzf_dense[0].as<char>())) return rc;
		u64 extent[2];
		V2M_HIP_TRY(ctx, hipMemcpyAsync(extent, ctx->d_bgzf_table.p, sizeof(extent), hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (extent[1] > cap - written)
			return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dst holds %llu bytes; the members need more (v2m_bgzf_bound(n) = %llu)", (unsigned long long) cap, (unsigned long long) v2m_bgzf_bound(n));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(static_cast<char *>(dst) + written, ctx->d_bgzf_dense[0].p, extent[1], hipMemcpyDeviceToHost, ctx->stream));
		V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		written += extent[1];
		done += chunk;
	}
	*n_out = written;
	return V2M_OK;
}

int v2m_bgzf_scan(const void *src, uint64_t n, uint64_t *n_members_out, uint64_t *n_bytes_out, int *ends_with_eof_out)
{
	if ((n && !src) || !n_members_out || !n_bytes_out || !ends_with_eof_out) return fail(nullptr, V2M_ERR_INVALID_ARGUMENT, "src or an output pointer is NULL");
	*n_members_out = 0;
	*n_bytes_out = 0;
	*ends_with_eof_out = 0;
	bgzf_members mem;
	std::string what;
	if (int const rc = bgzf_walk(static_cast<unsigned char const *>(src), n, mem, what)) return fail(nullptr, rc, "%s", what.c_str());
	*n_members_out = mem.isize.size();
	*n_bytes_out = mem.bytes;
	*ends_with_eof_out = mem.ends_with_eof ? 1 : 0;
	return V2M_OK;
}

// Slices of whole members (at most `slot` compressed and `slot` decompressed bytes each) go round two device slots and host slots 0 / 1
// (output) and 2 / 3 (input) of the ring: the host stages slice s + 1 into its pinned slot and queues its H2D copy and the D2H copy of
// slice s on copy_stream while slice s is inflated on stream; then it waits for slice s - 1's D2H copy, checks its statuses and copies it
// out to dst.  V2M_INFLATE_TIMING=1: where the call's time went, to stderr.
int v2m_bgzf_decompress(v2m_ctx *ctx, const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if ((n && !src) || !n_out) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "src or n_out is NULL");
	*n_out = 0;
	auto const now([] { return std::chrono::steady_clock::now(); });
	auto const since([&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); });
	auto const t_call(now());
	unsigned char const *const in(static_cast<unsigned char const *>(src));
	bgzf_members mem;
	{
		std::string what;
		if (int const rc = bgzf_walk(in, n, mem, what)) return fail(ctx, rc, "%s", what.c_str());
	}
	double const t_scan(since(t_call));
	if (cap < mem.bytes)
		return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dst holds %llu bytes; the members decompress to %llu", (unsigned long long) cap, (unsigned long long) mem.bytes);
	if (mem.bytes && !dst) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "dst is NULL");
	u64 const n_members(mem.isize.size());
	if (0 == n_members) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	// slices: [first member, end member), cut greedily
	char const *const slot_env(std::getenv("V2M_RING_SLOT_BYTES"));   // test knob: force small slices
	u64 const slot_target((slot_env && *slot_env) ? std::strtoull(slot_env, nullptr, 10) : (u64(64) << 20));
	// (no larger than the input needs: a small file does not set up 256 MB of pinned slots)
	u64 const slot(std::max<u64>(v2m::kBgzfSlotBytes, std::min(slot_target, (std::max<u64>(n, mem.bytes) + 0xffff) & ~u64(0xffff))));
	std::vector<u64> cut(1, 0);
	{
		u64 cin(0), cout(0);
		for (u64 k(0); k < n_members; ++k) {
			u64 const msize(mem.offsets[k + 1] - mem.offsets[k]);
			if (k > cut.back() && (cin + msize > slot || cout + mem.isize[k] > slot)) { cut.push_back(k); cin = 0; cout = 0; }
			cin += msize;
			cout += mem.isize[k];
		}
		cut.push_back(n_members);
	}
	u64 const n_slices(cut.size() - 1);
	u64 max_members(0);
	for (u64 s(0); s < n_slices; ++s) max_members = std::max(max_members, cut[s + 1] - cut[s]);
	u64 const table_bytes(2 * (max_members + 1) * sizeof(u64));
	u64 const in_slot((slot + 15) & ~u64(15)), status_bytes(max_members * sizeof(u32));
	if (int const rc = ensure_host_slots(ctx, 4, std::max(in_slot + table_bytes, ((slot + 15) & ~u64(15)) + status_bytes))) return rc;
	for (u64 i(0); i < 4; ++i) wait_released(ctx, *ctx->host_slots[i]);
	std::vector<u64> out_base(n_slices + 1, 0);
	for (u64 s(0); s < n_slices; ++s) {
		u64 b(out_base[s]);
		for (u64 k(cut[s]); k < cut[s + 1]; ++k) b += mem.isize[k];
		out_base[s + 1] = b;
	}

	bool const timing(nullptr != std::getenv("V2M_INFLATE_TIMING"));
	double t_stage(0), t_wait(0), t_copy_out(0), t_h2d(0), t_d2h(0);
	scoped_events tev;
	if (timing) V2M_HIP_TRY(ctx, tev.create(4 * n_slices));

	std::vector<u64> slice_out(n_slices, 0), slice_tab(n_slices, 0);
	// slice s in its input slots: its members' bytes, then (from slice_tab[s], the next multiple of 16) the member offsets and the output
	// offsets; only those bytes cross the link
	auto const stage([&](u64 s) -> int {   // slice s into its pinned input slot, and its H2D copy queued on copy_stream
		int const b(int(s & 1));
		u64 const k0(cut[s]), k1(cut[s + 1]), nm(k1 - k0);
		u64 const c0(mem.offsets[k0]), c1(mem.offsets[k1]);
		v2m_row_hold &slot_in(*ctx->host_slots[2 + b]);
		if (s >= 2) V2M_HIP_TRY(ctx, hipEventSynchronize(ctx->ev_inflate_in[b]));   // the H2D copy of slice s - 2 has left the slot
		auto const t0(now());
		V2M_POISON_HOST(slot_in.host.p, in_slot + table_bytes);
		host_copy(slot_in.host.p, in + c0, c1 - c0);
		u64 const tab_at((c1 - c0 + 15) & ~u64(15));                                        // <= in_slot
		slice_tab[s] = tab_at;
		u64 *const tab(reinterpret_cast<u64 *>(slot_in.host.as<char>() + tab_at));   // member offsets, then output offsets
		for (u64 k(k0); k <= k1; ++k) tab[k - k0] = mem.offsets[k] - c0;
		u64 o(0);
		for (u64 k(k0); k < k1; ++k) { tab[nm + 1 + k - k0] = o; o += mem.isize[k]; }
		tab[nm + 1 + nm] = o;
		slice_out[s] = o;
		t_stage += since(t0);
		if (s >= 2) V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute[b], 0));   // the kernel of slice s - 2 has read it
		V2M_HIP_TRY(ctx, ctx->d_inflate_in[b].ensure(in_slot + table_bytes));
		if (timing) V2M_HIP_TRY(ctx, hipEventRecord(tev[4 * s], ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_inflate_in[b].p, slot_in.host.p, tab_at + 2 * (nm + 1) * sizeof(u64), hipMemcpyHostToDevice, ctx->copy_stream));
		if (timing) V2M_HIP_TRY(ctx, hipEventRecord(tev[4 * s + 1], ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipEventRecord(ctx->ev_inflate_in[b], ctx->copy_stream));
		return V2M_OK;
	});
	auto const launch([&](u64 s) -> int {   // the kernel of slice s on stream
		int const b(int(s & 1));
		u64 const nm(cut[s + 1] - cut[s]);
		V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_inflate_in[b], 0));
		if (s >= 2) V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->host_slots[b]->copied, 0));   // the D2H copy of slice s - 2 is over
		V2M_HIP_TRY(ctx, ctx->d_inflate_out[b].ensure(std::max<u64>(16, in_slot)));
		V2M_HIP_TRY(ctx, ctx->d_inflate_status[b].ensure(status_bytes));
		char const *const d_in(ctx->d_inflate_in[b].as<char>());
		u64 const *const d_tab(reinterpret_cast<u64 const *>(d_in + slice_tab[s]));
		{
			timed_launch tl(ctx, V2M_KERNEL_INFLATE);
			hipLaunchKernelGGL(v2m::bgzf_inflate_kernel, dim3(unsigned(nm)), dim3(v2m::kInflateThreads), 0, ctx->stream,
				reinterpret_cast<unsigned char const *>(d_in), d_tab, d_tab + nm + 1, ctx->d_inflate_out[b].as<unsigned char>(), ctx->d_inflate_status[b].as<u32>());
			V2M_HIP_TRY(ctx, hipGetLastError());
		}
		V2M_HIP_TRY(ctx, hipEventRecord(ctx->ev_compute[b], ctx->stream));
		return V2M_OK;
	});
	auto const copy_back([&](u64 s) -> int {   // the D2H copy of slice s (bytes and statuses) queued on copy_stream
		int const b(int(s & 1));
		v2m_row_hold &slot_out(*ctx->host_slots[b]);
		V2M_HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute[b], 0));
		V2M_POISON_HOST(slot_out.host.p, in_slot + status_bytes);
		if (timing) V2M_HIP_TRY(ctx, hipEventRecord(tev[4 * s + 2], ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(slot_out.host.p, ctx->d_inflate_out[b].p, slice_out[s], hipMemcpyDeviceToHost, ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(slot_out.host.as<char>() + in_slot, ctx->d_inflate_status[b].p, (cut[s + 1] - cut[s]) * sizeof(u32), hipMemcpyDeviceToHost, ctx->copy_stream));
		if (timing) V2M_HIP_TRY(ctx, hipEventRecord(tev[4 * s + 3], ctx->copy_stream));
		V2M_HIP_TRY(ctx, hipEventRecord(slot_out.copied, ctx->copy_stream));
		return V2M_OK;
	});
	auto const finish([&](u64 s) -> int {   // slice s: statuses, then its bytes to dst
		v2m_row_hold &out_slot(*ctx->host_slots[s & 1]);
		auto const t0(now());
		V2M_HIP_TRY(ctx, hipEventSynchronize(out_slot.copied));
		t_wait += since(t0);
		u32 const *const st(reinterpret_cast<u32 const *>(out_slot.host.as<char>() + in_slot));
		for (u64 k(cut[s]); k < cut[s + 1]; ++k)
			if (st[k - cut[s]])
				return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "BGZF member %llu at compressed offset %llu: %s", (unsigned long long) k, (unsigned long long) mem.offsets[k],
					inflate_status_text(st[k - cut[s]]));
		auto const t1(now());
		host_copy(static_cast<char *>(dst) + out_base[s], out_slot.host.p, out_base[s + 1] - out_base[s]);
		t_copy_out += since(t1);
		return V2M_OK;
	});

	// copy_stream order: H2D 0, H2D 1, D2H 0, H2D 2, D2H 1, ...: the H2D copy of slice s + 1 and the D2H copy of slice s - 1 run under
	// the kernel of slice s, and the host copies slice s - 1 out meanwhile
	int rc(stage(0));
	u64 copied(0);
	for (u64 s(0); s < n_slices && V2M_OK == rc; ++s) {
		if (V2M_OK != (rc = launch(s))) break;
		if (s + 1 < n_slices && V2M_OK != (rc = stage(s + 1))) break;
		if (V2M_OK != (rc = copy_back(s))) break;
		copied = s + 1;
		if (s >= 1 && V2M_OK != (rc = finish(s - 1))) break;
	}
	if (V2M_OK == rc && copied) rc = finish(copied - 1);
	(void) hipStreamSynchronize(ctx->stream);
	(void) hipStreamSynchronize(ctx->copy_stream);
	if (V2M_OK != rc) return rc;
	if (timing) {
		for (u64 s(0); s < n_slices; ++s) {
			float a(0), b(0);
			if (hipSuccess == hipEventElapsedTime(&a, tev[4 * s], tev[4 * s + 1])) t_h2d += a / 1e3;
			if (hipSuccess == hipEventElapsedTime(&b, tev[4 * s + 2], tev[4 * s + 3])) t_d2h += b / 1e3;
		}
		std::fprintf(stderr, "[v2m_bgzf_decompress] %llu members, %llu -> %llu bytes in %llu slices: %.4f s in all; scan %.4f s, host staging %.4f s, "
			"H2D %.4f s, D2H %.4f s (device time), waiting for copies %.4f s, host copy out %.4f s\n", (unsigned long long) n_members, (unsigned long long) n,
			(unsigned long long) mem.bytes, (unsigned long long) n_slices, since(t_call), t_scan, t_stage, t_h2d, t_d2h, t_wait, t_copy_out);
	}
	*n_out = mem.bytes;
	return V2M_OK;
}


// ---- VCF scan (vcf_kernels.hpp) ----------------------------------------------------------------------

// One slice at a time, on the context's stream: its text into the slice buffer behind the carried line (plain: H2D from the caller's
// text; BGZF: the members through pinned slot 2, inflated by bgzf_inflate_kernel), the passes of vcf_kernels.hpp, the chunk into pinned
// slot 0, the callback.  The host waits for the device where the next launch's size depends on a count (lines, candidates' columns,
// head bytes and columns); nothing of the text crosses the link except the layout line, once.
int v2m_vcf_scan(v2m_ctx *ctx, const void *src, uint64_t n, const char *wanted_chr, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if ((n && !src) || !wanted_chr || !*wanted_chr || !layout || !chunk) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "src, wanted_chr, layout or chunk is NULL (or wanted_chr empty)");
	unsigned char const *const in(static_cast<unsigned char const *>(src));
	bool const bgzf(n >= 2 && 0x1f == in[0] && 0x8b == in[1]);
	bgzf_members mem;
	if (bgzf) {
		std::string what;
		if (int const rc = bgzf_walk(in, n, mem, what)) return fail(ctx, rc, "%s", what.c_str());
	}
	u64 const text_bytes(bgzf ? mem.bytes : n), n_members(bgzf ? mem.isize.size() : 0);
	if (0 == text_bytes) return V2M_OK;
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));

	char const *const slot_env(std::getenv("V2M_RING_SLOT_BYTES"));   // test knob: force small slices
	u64 const slot_target((slot_env && *slot_env) ? std::strtoull(slot_env, nullptr, 10) : (u64(64) << 20));
	u64 const slot(std::max<u64>(16, std::min<u64>({slot_target, u64(256) << 20, (text_bytes + 0xffff) & ~u64(0xffff)})));
	u64 const text_cap(slot + (bgzf ? v2m::kBgzfSlotBytes : 0));      // a slice's text at most; the carried line is no longer
	u64 const front((text_cap + 15) & ~u64(15));                      // the slice's new bytes begin here, the carried line ends here
	for (auto &b : ctx->d_vcf_text) { b.reset(); V2M_HIP_TRY(ctx, b.ensure(2 * front + 16)); }
	u32 const wanted_len(u32(std::strlen(wanted_chr)));
	V2M_HIP_TRY(ctx, ctx->d_vcf_wanted.ensure(wanted_len + 16));
	V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vcf_wanted.p, wanted_chr, wanted_len, hipMemcpyHostToDevice, ctx->stream));
	V2M_HIP_TRY(ctx, ctx->d_vcf_totals.ensure(64));

	bool have_layout(false);
	v2m_vcf_layout lay{};
	v2m::vcf_layout_view view{};
	u64 carry(0), first_line(0), consumed(0), next_member(0);         // consumed: plain bytes taken so far
	for (u64 s(0);; ++s) {
		unsigned char *const buf(ctx->d_vcf_text[s & 1].as<unsigned char>());
		// ---- the slice's new bytes
		u64 fresh(0);
		bool last(false);
		u64 k0(next_member), k1(next_member);
		if (bgzf) {
			while (k1 < n_members && (carry + fresh + mem.isize[k1] <= slot || (k1 == k0 && carry + mem.isize[k1] <= text_cap))) fresh += mem.isize[k1++];
			last = k1 == n_members;
			if (k1 == k0 && !last)
				return fail(ctx, V2M_ERR_UNSUPPORTED, "VCF line %llu is longer than a slice can hold (%llu bytes)", (unsigned long long) first_line + 1, (unsigned long long) slot);
			u64 const nm(k1 - k0);
			if (nm) {
				u64 const c0(mem.offsets[k0]), c1(mem.offsets[k1]);
				u64 const tab_at((c1 - c0 + 15) & ~u64(15)), tab_bytes(2 * (nm + 1) * sizeof(u64));
				if (int const rc = ensure_host_slots(ctx, 3, tab_at + tab_bytes)) return rc;
				for (u64 i(0); i < 3; ++i) wait_released(ctx, *ctx->host_slots[i]);
				char *const stage(ctx->host_slots[2]->host.as<char>());
				V2M_POISON_HOST(stage, tab_at + tab_bytes);
				host_copy(stage, in + c0, c1 - c0);
				u64 *const tab(reinterpret_cast<u64 *>(stage + tab_at));   // member offsets, then output offsets
				for (u64 k(k0); k <= k1; ++k) tab[k - k0] = mem.offsets[k] - c0;
				u64 o(0);
				for (u64 k(k0); k < k1; ++k) { tab[nm + 1 + k - k0] = o; o += mem.isize[k]; }
				tab[2 * nm + 1] = o;
				V2M_HIP_TRY(ctx, ctx->d_vcf_in.ensure(tab_at + tab_bytes));
				V2M_HIP_TRY(ctx, ctx->d_vcf_status.ensure(nm * sizeof(u32)));
				V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vcf_in.p, stage, tab_at + tab_bytes, hipMemcpyHostToDevice, ctx->stream));
				char const *const d_in(ctx->d_vcf_in.as<char>());
				u64 const *const d_tab(reinterpret_cast<u64 const *>(d_in + tab_at));
				{
					timed_launch tl(ctx, V2M_KERNEL_INFLATE);
					hipLaunchKernelGGL(v2m::bgzf_inflate_kernel, dim3(unsigned(nm)), dim3(v2m::kInflateThreads), 0, ctx->stream,
						reinterpret_cast<unsigned char const *>(d_in), d_tab, d_tab + nm + 1, buf + front, ctx->d_vcf_status.as<u32>());
					V2M_HIP_TRY(ctx, hipGetLastError());
				}
				std::vector<u32> status(nm);
				V2M_HIP_TRY(ctx, hipMemcpyAsync(status.data(), ctx->d_vcf_status.p, nm * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
				V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
				for (u64 k(0); k < nm; ++k)
					if (status[k])
						return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "BGZF member %llu at compressed offset %llu: %s", (unsigned long long) (k0 + k), (unsigned long long) mem.offsets[k0 + k],
							inflate_status_text(status[k]));
			}
			next_member = k1;
		} else {
			fresh = std::min(n - consumed, slot - std::min(slot, carry));
			last = consumed + fresh == n;
			if (0 == fresh && !last)
				return fail(ctx, V2M_ERR_UNSUPPORTED, "VCF line %llu is longer than a slice can hold (%llu bytes)", (unsigned long long) first_line + 1, (unsigned long long) slot);
			if (fresh) V2M_HIP_TRY(ctx, hipMemcpyAsync(buf + front, in + consumed, fresh, hipMemcpyHostToDevice, ctx->stream));
			consumed += fresh;
		}
		u64 const length(carry + fresh);                              // the slice's text: buf[front - carry, front + fresh)
		if (0 == length) break;                                       // (only at the end: nothing carried, nothing left)
		unsigned char const *const text(buf + front - carry);
		u32 const lead(u32(reinterpret_cast<uintptr_t>(text) & 15));
		unsigned char const *const base16(text - lead);
		u64 const end(lead + length);
		u32 const n_tiles(u32((end + v2m::kVcfTileBytes - 1) / v2m::kVcfTileBytes));

		u64 n_lines(0), tail_begin(0);
		u32 n_newlines(0);
		{
			// (one event pair per slice, closed after the slice's last kernel: the callbacks and the chunk's way to the host are not in it,
			// except, once, those of the chunk before the layout line)
			std::unique_ptr<timed_launch> tl(new timed_launch(ctx, V2M_KERNEL_VCF));
			// ---- the line index
			V2M_HIP_TRY(ctx, ctx->d_vcf_tiles.ensure(n_tiles * sizeof(u32)));
			V2M_HIP_TRY(ctx, ctx->d_vcf_tile_offsets.ensure((n_tiles + 1) * sizeof(u32)));
			hipLaunchKernelGGL(v2m::vcf_count_newlines_kernel, dim3(n_tiles), dim3(v2m::kVcfThreads), 0, ctx->stream, base16, lead, end, ctx->d_vcf_tiles.as<u32>());
			V2M_HIP_TRY(ctx, hipGetLastError());
			hipLaunchKernelGGL(v2m::vcf_scan_u32_kernel, dim3(1), dim3(v2m::kVcfScanThreads), 0, ctx->stream, ctx->d_vcf_tiles.as<u32>(), n_tiles, ctx->d_vcf_tile_offsets.as<u32>());
			V2M_HIP_TRY(ctx, hipGetLastError());
			V2M_HIP_TRY(ctx, hipMemcpyAsync(&n_newlines, ctx->d_vcf_tile_offsets.as<u32>() + n_tiles, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
			V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
			V2M_HIP_TRY(ctx, ctx->d_vcf_line_start.ensure((u64(n_newlines) + 2) * sizeof(u32)));
			// (a last line without '\n' is a line once the input has ended; whether there is one is known from the last line start)
			hipLaunchKernelGGL(v2m::vcf_line_starts_kernel, dim3(n_tiles), dim3(v2m::kVcfThreads), 0, ctx->stream, base16, lead, end,
				ctx->d_vcf_tile_offsets.as<u32>(), n_newlines, last ? 1u : 0u, ctx->d_vcf_line_start.as<u32>());
			V2M_HIP_TRY(ctx, hipGetLastError());
			{
				u32 tail(0);
				V2M_HIP_TRY(ctx, hipMemcpyAsync(&tail, ctx->d_vcf_line_start.as<u32>() + n_newlines, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
				V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
				if (tail > length) return fail(ctx, V2M_ERR_HIP, "VCF scan: a line start lies past the slice");
				tail_begin = tail;
			}
			n_lines = u64(n_newlines) + ((last && tail_begin < length) ? 1 : 0);
			if (0 == n_lines && !last && length >= slot)
				return fail(ctx, V2M_ERR_UNSUPPORTED, "VCF line %llu is longer than a slice can hold (%llu bytes)", (unsigned long long) first_line + 1, (unsigned long long) slot);

			if (n_lines) {
				// ---- heads
				V2M_HIP_TRY(ctx, ctx->d_vcf_lines.ensure(n_lines * sizeof(v2m_vcf_line)));
				V2M_HIP_TRY(ctx, ctx->d_vcf_gt_off.ensure(n_lines * sizeof(u32)));
				V2M_HIP_TRY(ctx, ctx->d_vcf_flags.ensure(n_lines * sizeof(u32)));
				V2M_HIP_TRY(ctx, ctx->d_vcf_tmp_begin.ensure(n_lines * sizeof(u32)));
				u32 const nl = u32(n_lines);
				u32 const *const d_ls(ctx->d_vcf_line_start.as<u32>());
				v2m_vcf_line *const d_lines(ctx->d_vcf_lines.as<v2m_vcf_line>());
				hipLaunchKernelGGL(v2m::vcf_head_kernel, dim3((nl + v2m::kVcfLinesPerHeadBlock - 1) / v2m::kVcfLinesPerHeadBlock), dim3(v2m::kVcfThreads), 0, ctx->stream,
					text, d_ls, nl, ctx->d_vcf_wanted.as<unsigned char>(), wanted_len, d_lines, ctx->d_vcf_gt_off.as<u32>(), ctx->d_vcf_flags.as<u32>());
				V2M_HIP_TRY(ctx, hipGetLastError());

				// ---- the layout, from the first line on the wanted chromosome
				u64 layout_at(n_lines);
				if (!have_layout) {
					std::vector<u32> flags(n_lines);
					V2M_HIP_TRY(ctx, hipMemcpyAsync(flags.data(), ctx->d_vcf_flags.p, n_lines * sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
					V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					layout_at = 0;
					while (layout_at < n_lines && !(flags[layout_at] & v2m::kVcfLineOnChromosome)) ++layout_at;
				}

				// lines [lo, hi) of the slice as one chunk: the genotypes of its candidates, its pools allocated in line order, the callback
				auto const deliver([&](u64 lo, u64 hi, bool closes) -> int {
					u32 const cl(u32(hi - lo));
					u32 const *const c_ls(d_ls + lo);
					v2m_vcf_line *const c_lines(d_lines + lo);
					u32 *const c_tmp_begin(ctx->d_vcf_tmp_begin.as<u32>() + lo);
					u64 totals[2] = {0, 0};
					if (have_layout) {
						hipLaunchKernelGGL(v2m::vcf_alloc_scan_kernel, dim3(1), dim3(v2m::kVcfScanThreads), 0, ctx->stream, c_lines, cl, 1u, c_tmp_begin, ctx->d_vcf_totals.as<u64>());
						V2M_HIP_TRY(ctx, hipGetLastError());
						V2M_HIP_TRY(ctx, hipMemcpyAsync(totals, ctx->d_vcf_totals.p, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
						V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
						if (totals[0] > u64(cl) * v2m::kVcfMaxAlts) return fail(ctx, V2M_ERR_HIP, "VCF scan: bad candidate column count");
						V2M_HIP_TRY(ctx, ctx->d_vcf_tmp_columns.ensure(std::max<u64>(16, totals[0] * lay.words_per_column * sizeof(u64))));
						if (totals[0]) {
							// the instance whose LDS columns are just wide enough
							auto const launch([&](auto kernel) {
								hipLaunchKernelGGL(kernel, dim3(cl), dim3(64), 0, ctx->stream, text, c_ls, cl, c_lines, ctx->d_vcf_gt_off.as<u32>() + lo,
									c_tmp_begin, view, ctx->d_vcf_tmp_columns.as<u64>());
							});
							if (lay.words_per_column <= 4) launch(v2m::vcf_genotype_kernel<4>);
							else if (lay.words_per_column <= 32) launch(v2m::vcf_genotype_kernel<32>);
							else if (lay.words_per_column <= 128) launch(v2m::vcf_genotype_kernel<128>);
							else launch(v2m::vcf_genotype_kernel<v2m::kVcfMaxWordsPerColumn>);
							V2M_HIP_TRY(ctx, hipGetLastError());
						}
					}
					hipLaunchKernelGGL(v2m::vcf_alloc_scan_kernel, dim3(1), dim3(v2m::kVcfScanThreads), 0, ctx->stream, c_lines, cl, 0u, c_tmp_begin, ctx->d_vcf_totals.as<u64>());
					V2M_HIP_TRY(ctx, hipGetLastError());
					V2M_HIP_TRY(ctx, hipMemcpyAsync(totals, ctx->d_vcf_totals.p, sizeof(totals), hipMemcpyDeviceToHost, ctx->stream));
					V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					u64 const head_bytes(totals[0]), n_columns(totals[1]);
					if (head_bytes > length || n_columns > u64(cl) * v2m::kVcfMaxAlts || (n_columns && !have_layout)) return fail(ctx, V2M_ERR_HIP, "VCF scan: bad pool sizes");
					u64 const column_bytes(n_columns * lay.words_per_column * sizeof(u64));
					V2M_HIP_TRY(ctx, ctx->d_vcf_heads.ensure(std::max<u64>(16, head_bytes)));
					V2M_HIP_TRY(ctx, ctx->d_vcf_columns.ensure(std::max<u64>(16, column_bytes)));
					if (!ctx->d_vcf_tmp_columns.p) V2M_HIP_TRY(ctx, ctx->d_vcf_tmp_columns.ensure(16));
					hipLaunchKernelGGL(v2m::vcf_gather_kernel, dim3(cl), dim3(v2m::kVcfThreads), 0, ctx->stream, text, c_ls, cl, c_lines, c_tmp_begin,
						ctx->d_vcf_tmp_columns.as<u64>(), u32(lay.words_per_column), head_bytes, n_columns, ctx->d_vcf_heads.as<unsigned char>(), ctx->d_vcf_columns.as<u64>());
					V2M_HIP_TRY(ctx, hipGetLastError());
					if (closes) tl.reset();

					u64 const columns_at((u64(cl) * sizeof(v2m_vcf_line) + 15) & ~u64(15)), heads_at(columns_at + ((column_bytes + 15) & ~u64(15)));
					u64 const out_bytes(heads_at + head_bytes + 16);
					if (int const rc = ensure_host_slots(ctx, 1, out_bytes)) return rc;
					wait_released(ctx, *ctx->host_slots[0]);
					char *const host(ctx->host_slots[0]->host.as<char>());
					V2M_POISON_HOST(host, out_bytes);
					V2M_HIP_TRY(ctx, hipMemcpyAsync(host, c_lines, u64(cl) * sizeof(v2m_vcf_line), hipMemcpyDeviceToHost, ctx->stream));
					if (column_bytes) V2M_HIP_TRY(ctx, hipMemcpyAsync(host + columns_at, ctx->d_vcf_columns.p, column_bytes, hipMemcpyDeviceToHost, ctx->stream));
					if (head_bytes) V2M_HIP_TRY(ctx, hipMemcpyAsync(host + heads_at, ctx->d_vcf_heads.p, head_bytes, hipMemcpyDeviceToHost, ctx->stream));
					V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					v2m_vcf_chunk c{};
					c.first_line = first_line + lo;
					c.n_lines = cl;
					c.lines = reinterpret_cast<v2m_vcf_line const *>(host);
					c.heads = host + heads_at;
					c.head_bytes = head_bytes;
					c.columns = reinterpret_cast<u64 const *>(host + columns_at);
					c.n_columns = n_columns;
					c.words_per_column = have_layout ? lay.words_per_column : 0;
					if (0 != chunk(user, &c)) return fail(ctx, V2M_ERR_SINK, "chunk callback asked to stop at line %llu", (unsigned long long) c.first_line);
					return V2M_OK;
				});

				if (layout_at < n_lines) {
					// the lines before the layout line are a chunk of their own: the caller has seen the #CHROM line when `layout` runs
					if (layout_at) if (int const rc = deliver(0, layout_at, false)) return rc;
					u32 be[2];
					V2M_HIP_TRY(ctx, hipMemcpyAsync(be, d_ls + layout_at, sizeof(be), hipMemcpyDeviceToHost, ctx->stream));
					V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					if (be[0] >= be[1] || be[1] - 1 > length) return fail(ctx, V2M_ERR_HIP, "VCF scan: bad line index");
					u32 const line_len(be[1] - 1 - be[0]);
					std::vector<char> line(u64(line_len) + 1);
					V2M_HIP_TRY(ctx, hipMemcpyAsync(line.data(), text + be[0], line_len, hipMemcpyDeviceToHost, ctx->stream));
					V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					if (0 != layout(user, first_line + layout_at, line.data(), line_len, &lay)) return fail(ctx, V2M_ERR_SINK, "layout callback asked to stop");
					if (lay.n_rows > v2m::kVcfMaxRows || lay.words_per_column > v2m::kVcfMaxWordsPerColumn)
						return fail(ctx, V2M_ERR_UNSUPPORTED, "VCF scan: %u chromosome copies (%llu words per column); at most %u (%u words) are supported", lay.n_rows,
							(unsigned long long) lay.words_per_column, v2m::kVcfMaxRows, v2m::kVcfMaxWordsPerColumn);
					if ((lay.n_samples && (!lay.copy_begin || (lay.copy_begin[lay.n_samples] && !lay.row_lookup))) || u64(lay.n_rows) > 64 * lay.words_per_column)
						return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "VCF scan: incomplete layout");
					u32 n_copies(0);
					for (u32 i(0); i < lay.n_samples; ++i) {
						if (lay.copy_begin[i + 1] < lay.copy_begin[i]) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "VCF scan: copy_begin decreases at sample %u", i);
						n_copies = lay.copy_begin[i + 1];
					}
					for (u32 i(lay.n_samples ? lay.copy_begin[0] : 0); i < n_copies; ++i)
						if (lay.row_lookup[i] < -1 || lay.row_lookup[i] >= std::int64_t(lay.n_rows)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "VCF scan: row_lookup[%u] is outside the rows", i);
					u64 const cb_bytes(((u64(lay.n_samples) + 1) * sizeof(u32) + 15) & ~u64(15));
					V2M_HIP_TRY(ctx, ctx->d_vcf_layout.ensure(cb_bytes + std::max<u64>(16, u64(n_copies) * sizeof(std::int32_t))));
					u32 const zero(0);
					V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vcf_layout.p, lay.n_samples ? lay.copy_begin : &zero, (u64(lay.n_samples) + 1) * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
					if (n_copies) V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vcf_layout.as<char>() + cb_bytes, lay.row_lookup, u64(n_copies) * sizeof(std::int32_t), hipMemcpyHostToDevice, ctx->stream));
					V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
					view.copy_begin = ctx->d_vcf_layout.as<u32>();
					view.row_lookup = reinterpret_cast<std::int32_t const *>(ctx->d_vcf_layout.as<char>() + cb_bytes);
					view.n_samples = lay.n_samples;
					view.n_rows = lay.n_rows;
					view.words_per_column = u32(lay.words_per_column);
					have_layout = true;
					if (int const rc = deliver(layout_at, n_lines, true)) return rc;
				}
				else if (int const rc = deliver(0, n_lines, true)) return rc;
			}
		}

		// ---- the line the slice ends in goes in front of the next slice's bytes (the other buffer)
		u64 const next_carry(last ? 0 : length - tail_begin);
		if (next_carry) {
			if (next_carry > front) return fail(ctx, V2M_ERR_UNSUPPORTED, "VCF line %llu is longer than a slice can hold (%llu bytes)", (unsigned long long) (first_line + n_lines + 1), (unsigned long long) slot);
			V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_vcf_text[(s + 1) & 1].as<unsigned char>() + front - next_carry, text + tail_begin, next_carry, hipMemcpyDeviceToDevice, ctx->stream));
		}
		first_line += n_lines;
		carry = next_carry;
		if (last) break;
	}
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return V2M_OK;
}


// ---- checksums ------------------------------------------------------------------------------

int v2m_checksum_rows_device(v2m_ctx *ctx, const void *d_rows, uint64_t row_pitch, uint64_t n_rows, uint64_t length, const uint64_t *lengths, uint64_t *checksums_out)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (0 == n_rows) return V2M_OK;
	if (!d_rows || !checksums_out || ((uintptr_t) d_rows & 7) || (row_pitch & 7)) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "bad checksum arguments");
	V2M_HIP_TRY(ctx, hipSetDevice(ctx->device));
	V2M_HIP_TRY(ctx, ctx->d_sums.ensure(n_rows * 8));
	V2M_HIP_TRY(ctx, hipMemsetAsync(ctx->d_sums.p, 0, n_rows * 8, ctx->stream));
	u64 max_len(length);
	u64 const *d_lengths(nullptr);
	if (lengths) {
		max_len = *std::max_element(lengths, lengths + n_rows);
		V2M_HIP_TRY(ctx, ctx->d_lengths.ensure(n_rows * 8));
		V2M_HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lengths.p, lengths, n_rows * 8, hipMemcpyHostToDevice, ctx->stream));
		d_lengths = ctx->d_lengths.as<u64>();
	}
	for (u64 r(0); r < n_rows; ++r) {
		u64 const len(lengths ? lengths[r] : length);
		if (len > row_pitch) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "row %llu is longer than the pitch", (unsigned long long) r);
	}
	u64 const words_per_block(256 * 32);
	u64 const n_words((max_len + 7) / 8);
	u64 const gx(std::max<u64>(1, (n_words + words_per_block - 1) / words_per_block));
	for (u64 r0(0); r0 < n_rows; r0 += 32768) {
		u64 const nr(std::min<u64>(32768, n_rows - r0));
		hipLaunchKernelGGL(v2m::checksum_rows_kernel, dim3(unsigned(gx), unsigned(nr)), dim3(256), 0, ctx->stream,
			static_cast<char const *>(d_rows) + r0 * row_pitch, row_pitch, d_lengths ? d_lengths + r0 : nullptr, length, words_per_block,
			ctx->d_sums.as<unsigned long long>() + r0);
		V2M_HIP_TRY(ctx, hipGetLastError());
	}
	V2M_HIP_TRY(ctx, hipMemcpyAsync(checksums_out, ctx->d_sums.p, n_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return V2M_OK;
}


// ---- profiling ------------------------------------------------------------------------------

int v2m_profile_enable(v2m_ctx *ctx, int enabled)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	ctx->profiling = (0 != enabled);
	return V2M_OK;
}

int v2m_profile_reset(v2m_ctx *ctx)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	for (auto &v : ctx->events) {
		ctx->free_events.insert(ctx->free_events.end(), v.begin(), v.end());
		v.clear();
	}
	return V2M_OK;
}

int v2m_profile_get(v2m_ctx *ctx, int kernel, uint64_t *launches_out, double *total_ms_out)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (kernel < 0 || kernel >= V2M_KERNEL_LIMIT) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "unknown kernel id %d", kernel);
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	double total(0);
	for (auto const &e : ctx->events[kernel]) {
		float ms(0);
		V2M_HIP_TRY(ctx, hipEventElapsedTime(&ms, e.begin, e.end));
		total += ms;
	}
	if (launches_out) *launches_out = ctx->events[kernel].size();
	if (total_ms_out) *total_ms_out = total;
	return V2M_OK;
}

int v2m_profile_get_launches(v2m_ctx *ctx, int kernel, double *ms_out, uint64_t capacity, uint64_t *launches_out)
{
	if (!ctx) return V2M_ERR_INVALID_ARGUMENT;
	if (kernel < 0 || kernel >= V2M_KERNEL_LIMIT) return fail(ctx, V2M_ERR_INVALID_ARGUMENT, "unknown kernel id %d", kernel);
	V2M_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	auto const &ev(ctx->events[kernel]);
	for (u64 i(0); i < ev.size() && i < capacity && ms_out; ++i) {
		float ms(0);
		V2M_HIP_TRY(ctx, hipEventElapsedTime(&ms, ev[i].begin, ev[i].end));
		ms_out[i] = ms;
	}
	if (launches_out) *launches_out = ev.size();
	return V2M_OK;
}

} // extern "C"
