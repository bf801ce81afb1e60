/*
 * v2m_hip.h -- C ABI of the MI355X (gfx950) haplotype-splice path for vcf2multialign.
 *
 * Drop-in boundary for ONE hot path of tsnorri/vcf2multialign: the per-row
 * reference+ALT splice (output_sequence) batched over the rows of one A2M file, and the
 * bit-packed path-matrix transpose.  The C++ host keeps parsing the VCF, building the
 * variant_graph and writing the A2M file; everything between "graph built" and "row
 * bytes ready" happens on the GPU behind these entry points.
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   v2m_transpose_bits[_device]   transpose_matrix()            include/vcf2multialign/transpose_matrix.hh:14
 *                                                                libvcf2multialign/transpose_matrix.cc:41-109
 *                                                                (call site libvcf2multialign/variant_graph.cc:453)
 *   v2m_upload_graph              the read-only view of          include/vcf2multialign/variant_graph.hh:57-66
 *                                 variant_graph + ref_seq that
 *                                 output_sequence() walks
 *   v2m_splice_rows[_device]      output_sequence() called once  include/vcf2multialign/sequence_writer.hh:49-56
 *                                 per row by                     libvcf2multialign/sequence_writer.cc:22-85
 *                                 haplotype_output::output_a2m   libvcf2multialign/haplotype_output.cc:38-82
 *                                 and founder_sequence_greedy_   libvcf2multialign/founder_sequence_greedy_output.cc:515-550
 *                                 output::output_a2m
 *   v2m_row_batch                 sequence_writing_delegate      include/vcf2multialign/sequence_writer.hh:16-36
 *                                 (chromosome_copy_index, and    libvcf2multialign/haplotype_output.cc:22-32
 *                                 the founder delegate's copy    libvcf2multialign/founder_sequence_greedy_output.cc:78-115
 *                                 switch at cut nodes)
 *   v2m_upload_path_slice /       transpose_matrix() at its one  libvcf2multialign/variant_graph.cc:453
 *   v2m_upload_path_blocks /      call site, for one GPU's       include/vcf2multialign/variant_graph.hh:62-63
 *   v2m_bind_path_matrix_device   chromosome copies (or all)
 *   v2m_pbwt_cut_trials[_streamed] the edge-by-edge part of      include/vcf2multialign/pbwt.hh:77-134
 *   v2m_pbwt_cut_records          find_cut_positions() and       libvcf2multialign/find_cut_positions.cc:126-176
 *                                 find_matchings() (optional)    libvcf2multialign/founder_sequence_greedy_output.cc:208-251
 *
 * V2M_ABI_VERSION: 1 = round 1 (transpose, graph, rows); 2 = + v2m_upload_path_slice, v2m_alloc_output / v2m_free_output,
 * v2m_profile_get_launches (v2m_bind_path_matrix_device followed without a step); 3 = + v2m_upload_path_blocks (and then
 * v2m_pbwt_cut_trials, v2m_pbwt_cut_records); 4 = + v2m_pbwt_cut_trials_streamed; 5 = + v2m_splice_rows_held / v2m_row_release (rows a
 * sink may keep until it says so).  Entries have only ever been added.  V2M_SPLICE_BGZF, v2m_bgzf_compress, v2m_bgzf_bound and
 * v2m_bgzf_frame_stored were added without a new version, and so were v2m_set_column_window and v2m_window_length, and
 * v2m_bgzf_scan and v2m_bgzf_decompress (with V2M_KERNEL_INFLATE), and v2m_vcf_scan (with V2M_KERNEL_VCF): a caller probes for them by symbol.
 * The window-set calls (v2m_window_set_layout, v2m_set_window_set, v2m_splice_window_set[_device]) were added the same way, and so was
 * v2m_row_ops (with v2m_aln_op, v2m_ops_sink_fn and the V2M_KERNEL_ROW_OPS_* ids), and v2m_splice_window_set_distinct (with
 * v2m_distinct_sink_fn and the V2M_KERNEL_DISTINCT_* ids), and v2m_column_counts / v2m_column_counts_device (with v2m_column_count,
 * v2m_column_counts_sink_fn, the V2M_COUNTS_* flags and the V2M_KERNEL_COLUMN_* ids), and v2m_pair_distances / v2m_pair_distances_device
 * (with v2m_pair_distances_info, V2M_DIST_ACGT_ONLY and V2M_PAIR_DISTANCES_MAX_ROWS; no kernel ids: the info carries their times), and
 * v2m_variable_sites / v2m_variable_sites_device (with v2m_variable_sites_info, the two sink types and V2M_SITES_SNP; no kernel ids either),
 * and v2m_nj_tree / v2m_nj_tree_of_distances (with v2m_nj_node, v2m_nj_tree_info, V2M_NJ_NONE and V2M_NJ_MAX_ROWS; no kernel ids),
 * and v2m_pair_distances_weighted / v2m_bootstrap_distances / v2m_nj_bootstrap (with v2m_nj_bootstrap_info and
 * V2M_NJ_BOOTSTRAP_MAX_REPLICATES; no kernel ids).
 *
 * Conventions
 *   - Plain C: pointers + sizes, no exceptions, no C++/torch types.  Every function that can
 *     fail returns a V2M_* status; v2m_last_error() gives the message.
 *   - All graph integers are uint64_t exactly as in the reference (variant_graph.hh:38-40);
 *     the library narrows to 32 bits on upload and rejects graphs that do not fit
 *     (V2M_ERR_UNSUPPORTED).
 *   - Bit matrices: column-major, one column = n_rows/64 consecutive uint64_t words, row r of a
 *     column in word r/64 at bit r%64 (LSB first).  Dimensions are multiples of 64.
 *   - One ctx per GPU, driven by one host thread.  The graph is uploaded once and reused.
 *   - There is NO CPU fallback: without a usable HIP device v2m_ctx_create() fails.
 */
#ifndef V2M_HIP_H
#define V2M_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define V2M_ABI_VERSION 5

enum {
	V2M_OK = 0,
	V2M_ERR_INVALID_ARGUMENT = 1, /* null pointer, zero-sized where not allowed, bad flag */
	V2M_ERR_PRECONDITION = 2,     /* what the reference asserts: dims % 64, graph invariants, cut nodes */
	V2M_ERR_UNSUPPORTED = 3,      /* valid input outside what this build handles (e.g. > 32-bit positions) */
	V2M_ERR_NO_DEVICE = 4,        /* no HIP device / wrong architecture */
	V2M_ERR_HIP = 5,              /* a HIP runtime call failed */
	V2M_ERR_OUT_OF_MEMORY = 6,
	V2M_ERR_SINK = 7,             /* the sink callback returned non-zero */
	V2M_ERR_STATE = 8             /* call order: no graph uploaded, no path matrix set, ... */
};

/* sequence_writing_delegate::PLOIDY_MAX (sequence_writer.hh:23-25): "follow REF edges only". */
#define V2M_PLOIDY_MAX UINT32_MAX

/* flags of v2m_splice_rows* */
#define V2M_SPLICE_UNALIGNED 0x1u /* should_output_unaligned (sequence_writer.cc:80): no '-' padding.  Bytes are opaque to the
                                   * walk (sequence_writer.cc:73-74 streams whatever the FASTA / VCF held) and aligned mode keeps
                                   * every byte value; the unaligned kernels use byte 0 as their padding marker, so a graph whose
                                   * ref_seq or label pool holds a NUL byte is refused in this mode (V2M_ERR_UNSUPPORTED) rather
                                   * than written without it. */
#define V2M_SPLICE_BGZF 0x2u      /* v2m_splice_rows only (may be combined with V2M_SPLICE_UNALIGNED): the sink receives, per row and
                                   * in batch order, the complete BGZF members of that row's body instead of the body (format below).
                                   * v2m_splice_rows_held returns V2M_ERR_UNSUPPORTED with it, v2m_splice_rows_device
                                   * V2M_ERR_INVALID_ARGUMENT. */

typedef struct v2m_ctx v2m_ctx;

/* ---- context ---------------------------------------------------------------------------- */

/* Binds to HIP device `device_id`, creates the library's stream.  Fails with V2M_ERR_NO_DEVICE
 * when there is no usable gfx950 device. */
int v2m_ctx_create(int device_id, v2m_ctx **ctx_out);
void v2m_ctx_destroy(v2m_ctx *ctx);

/* Message of the last failure on this ctx (or, with ctx == NULL, of the last failed
 * ctx-less call on this thread: v2m_ctx_create, v2m_bgzf_scan).  Never NULL. */
const char *v2m_last_error(const v2m_ctx *ctx);

/* Blocks until everything queued on the ctx's stream has finished. */
int v2m_ctx_synchronize(v2m_ctx *ctx);

/* The hipStream_t all kernels of this ctx are launched on (for event timing by the caller). */
void *v2m_ctx_stream(v2m_ctx *ctx);

/* Human-readable note on what the context has auto-tuned so far (e.g. the store flavour of the aligned
 * splice, calibrated on the first >= 1 GiB launch).  Never NULL; empty before any tuning. */
const char *v2m_ctx_info(const v2m_ctx *ctx);

uint32_t v2m_abi_version(void);

/* ---- transpose_matrix ------------------------------------------------------------------- */

/* dst(c, r) = src(r, c).  src has n_rows x n_cols bits, dst n_cols x n_rows; both column-major
 * uint64 words as above; dst holds n_rows*n_cols/64 words and is fully overwritten.
 * n_cols == 0 is a no-op returning V2M_OK (transpose_matrix.cc:48-49); dimensions that are
 * not multiples of 64 return V2M_ERR_PRECONDITION (asserted at transpose_matrix.cc:53-54).
 * Host-pointer form: copies in, transposes on the GPU, copies out, synchronous. */
int v2m_transpose_bits(v2m_ctx *ctx, const uint64_t *src_words, uint64_t n_rows, uint64_t n_cols, uint64_t *dst_words);

/* Device-pointer form: both buffers already in HBM (8-byte aligned, non-overlapping);
 * asynchronous on the ctx's stream. */
int v2m_transpose_bits_device(v2m_ctx *ctx, const void *d_src_words, uint64_t n_rows, uint64_t n_cols, void *d_dst_words);

/* ---- variant_graph view ----------------------------------------------------------------- */

/* Raw view of the variant_graph fields output_sequence() reads (variant_graph.hh:57-63),
 * with alt_edge_labels flattened to CSR.  All pointers are host pointers owned by the caller
 * and only read during v2m_upload_graph(). */
typedef struct v2m_graph_view {
	uint64_t node_count;                 /* reference_positions.size() (>= 1; last node = sink) */
	uint64_t edge_count;                 /* alt_edge_targets.size() */
	const uint64_t *reference_positions; /* [node_count]  strictly increasing                   */
	const uint64_t *aligned_positions;   /* [node_count]  MSA co-ordinates                      */
	const uint64_t *alt_edge_targets;    /* [edge_count]  node ids                              */
	const uint64_t *alt_edge_count_csum; /* [node_count + 1]; edges of node n = [csum[n], csum[n+1]) */
	const uint64_t *alt_edge_label_offsets; /* [edge_count + 1] offsets into alt_edge_label_bytes */
	const char *alt_edge_label_bytes;
	/* paths_by_chrom_copy_and_edge: rows = edges (padded to path_rows), cols = chromosome copies
	 * (padded to path_cols).  May be NULL when the matrix is supplied later with
	 * v2m_set_paths_device(). */
	const uint64_t *paths_by_chrom_copy_and_edge;
	uint64_t path_rows; /* >= edge_count, multiple of 64 (0 allowed when edge_count == 0) */
	uint64_t path_cols; /* multiple of 64 */
} v2m_graph_view;

/* Validates the invariants output_sequence() relies on (V2M_ERR_PRECONDITION otherwise),
 * narrows to 32 bits, uploads graph + reference, and precomputes the device-side tables
 * (edge source nodes, per-edge aligned spans, the gap-aligned REF row, per-tile edge ranges).
 * Replaces any previously uploaded graph.  Synchronous. */
int v2m_upload_graph(v2m_ctx *ctx, const v2m_graph_view *graph, const char *ref_seq, uint64_t ref_len);

/* Uses a path matrix that already lives in HBM (e.g. the output of v2m_transpose_bits_device)
 * as paths_by_chrom_copy_and_edge of the uploaded graph.  The buffer is BORROWED: it must stay
 * valid and unchanged until the next upload/set or ctx destruction. */
int v2m_set_paths_device(v2m_ctx *ctx, const void *d_words, uint64_t path_rows, uint64_t path_cols);

/* One GPU's share of the path matrix when chromosome copies are sharded over several GPUs (rows are independent,
 * haplotype_output.cc:62-81; the graph and reference are replicated with v2m_upload_graph, the matrix is not).
 * `paths_by_edge_and_chrom_copy` is the WHOLE host-resident transpose input (variant_graph.hh:62: n_rows = chromosome
 * copies, n_cols = ALT edges, both multiples of 64, column-major as above) as build_variant_graph leaves it just before
 * its transpose_matrix call (variant_graph.cc:453).  Only the bits of copies [first_copy, first_copy + n_copies) are
 * moved to this GPU -- bytes [first_copy / 8, ..) of every column, a strided 2-D copy; first_copy must be a multiple
 * of 8 -- zero-padded to a multiple of 64 copies, transposed THERE (the same kernels as v2m_transpose_bits_device) and
 * bound as paths_by_chrom_copy_and_edge of the uploaded graph: n_cols rows (edges) x 64 * ceil(n_copies / 64) columns,
 * column j = copy first_copy + j.  Row batches for this ctx then use copy indices relative to first_copy.
 * first_copy = 0, n_copies = n_rows is the unsharded case: upload + transpose + bind without the matrix ever coming
 * back to the host.  The result is owned by the ctx.  Synchronous. */
int v2m_upload_path_slice(v2m_ctx *ctx, const uint64_t *paths_by_edge_and_chrom_copy, uint64_t n_rows, uint64_t n_cols, uint64_t first_copy, uint64_t n_copies);

/* The same for a GPU whose chromosome copies are not one contiguous range but every stride_copies-th block of block_copies
 * copies: copies first_copy + j * stride_copies + [0, block_copies) for j = 0, 1, ..., clipped to copy_end (first_copy,
 * block_copies and stride_copies multiples of 8).  Column l of the bound matrix is copy
 * first_copy + (l / block_copies) * stride_copies + l % block_copies, and row batches for this ctx use those local indices.
 * This is how several GPUs share an output that has to leave in row order (a pipe, an unaligned A2M file,
 * haplotype_output.cc:62-81 with sequence_writer.cc:80): with blocks dealt round-robin, GPU k produces rows
 * k * block, ..., then (k + G) * block, ... while the others produce the blocks in between, and a single writer can drain
 * them in order from buffers that hold a few rows per GPU; contiguous shards would leave all but one GPU waiting.
 * v2m_upload_path_slice(first, n) is the one-block case.  Synchronous. */
int v2m_upload_path_blocks(v2m_ctx *ctx, const uint64_t *paths_by_edge_and_chrom_copy, uint64_t n_rows, uint64_t n_cols, uint64_t first_copy, uint64_t block_copies, uint64_t stride_copies, uint64_t copy_end);

/* The same for a transpose input that already lives in HBM (n_rows copies x n_cols edges, dense column-major words as
 * above, e.g. generated or assembled on the device): transposes it into a ctx-owned copy of paths_by_chrom_copy_and_edge and
 * binds that -- the one-call form of v2m_transpose_bits_device() + v2m_set_paths_device().  The owned copy is laid out for
 * the GPU (every chromosome copy's column starts on a 128-byte line), which a caller-visible destination cannot be, so
 * this is the faster of the two ways.  Asynchronous on the ctx's stream; the source may be reused once the call's work
 * has finished (v2m_ctx_synchronize()). */
int v2m_bind_path_matrix_device(v2m_ctx *ctx, const void *d_paths_by_edge_and_chrom_copy, uint64_t n_rows, uint64_t n_cols);

/* aligned_positions.back(): the length of every aligned row. 0 before an upload.  (A column window does not change it.) */
uint64_t v2m_aligned_length(const v2m_ctx *ctx);
/* The row pitch the library itself uses in aligned mode (aligned length rounded up to 256: rows then start on
 * 256-B boundaries).  v2m_splice_rows_device accepts any multiple of 16 that is >= the aligned length rounded up to 16.
 * With a column window (v2m_set_column_window) both rules take the window's length instead of the aligned length. */
uint64_t v2m_min_row_pitch(const v2m_ctx *ctx);

/* ---- rows -------------------------------------------------------------------------------- */

/* A batch of output rows, i.e. one sequence_writing_delegate per row:
 *   - row i with no cuts follows chromosome copy copy_index[i] for the whole walk
 *     (haplotype_output.cc:22-32); V2M_PLOIDY_MAX = the REF row (haplotype_output.cc:55).
 *   - row i with cuts [cut_offsets[i], cut_offsets[i+1]) starts as V2M_PLOIDY_MAX and switches to
 *     cut_copies[k] when the walk visits node cut_nodes[k] (founder_sequence_greedy_output.cc:106-114).
 *     Cut nodes must be strictly increasing and must not lie strictly inside any ALT edge's
 *     (source, target) node span -- the reference asserts this at :108; violating batches are
 *     rejected with V2M_ERR_PRECONDITION.  cut_copies may be V2M_PLOIDY_MAX.
 * cut_offsets == NULL means no row has cuts.  Copy indices must be < path_cols. */
typedef struct v2m_row_batch {
	uint64_t n_rows;
	const uint32_t *copy_index;  /* [n_rows] */
	const uint64_t *cut_offsets; /* [n_rows + 1] or NULL */
	const uint64_t *cut_nodes;   /* [cut_offsets[n_rows]] */
	const uint32_t *cut_copies;  /* [cut_offsets[n_rows]] */
} v2m_row_batch;

/* Receives one finished row body: exactly the bytes output_sequence() would have streamed
 * after the optional '>'id'\n' header and before the caller's '\n' (haplotype_output.cc:57,76).
 * `bytes` is library-owned pinned memory, valid only during the call.  Rows arrive in batch
 * order, one call per row, on the calling thread.  Return non-zero to abort (V2M_ERR_SINK). */
typedef int (*v2m_sink_fn)(void *user, uint64_t row_index, const char *bytes, uint64_t length);

/* Splices every row of the batch on the GPU and hands the bodies to `sink` in order.
 * Works through the batch in device-sized slices, overlapping the D2H copy of one slice with
 * the kernels of the next.  Synchronous. */
int v2m_splice_rows(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_sink_fn sink, void *user);

/* The same rows for a sink that does not finish with a row inside the call -- one that queues it for a pool of writer threads
 * (output.cc:47-76 with more than one thread behind the file descriptor: a file per sequence, haplotype_output.cc:85-132, scales
 * with writers where one writer on one stream does not).  `bytes` stays valid, in a pinned slot of the library's, until the sink
 * calls v2m_row_release(hold) -- once per accepted row, from any thread, during or after the sink call.  Rows still arrive in batch
 * order on the calling thread, and the call goes on launching slices and copies meanwhile; a slot is copied into again only when
 * every row of it has been released.  n_slots (2 ... 64) pinned slots of the slice size v2m_splice_rows uses (512 MB for batches
 * of 8 GB and more, else 128 MB) are allocated on first use and kept by the ctx: rows in writers' hands + rows crossing the link
 * + rows being delivered all need a slot, so n_slots = writers' rows / rows per slot + 2 is the least that keeps the link busy.
 * A sink that returns non-zero has NOT accepted that row (it must not release it) and ends the call with V2M_ERR_SINK.
 * The call returns only when every accepted row has been released, also after an error.  Synchronous. */
typedef struct v2m_row_hold v2m_row_hold;
typedef int (*v2m_hold_sink_fn)(void *user, uint64_t row_index, const char *bytes, uint64_t length, v2m_row_hold *hold);
int v2m_splice_rows_held(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, uint32_t n_slots, v2m_hold_sink_fn sink, void *user);
void v2m_row_release(v2m_row_hold *hold);

/* Device-resident form: row i is written to d_out + i * row_pitch and stays in HBM.
 * Aligned mode: every row has v2m_aligned_length() bytes; row_pitch a multiple of 16 and >= the aligned length
 * rounded up to 16 (v2m_min_row_pitch() is what the library uses itself); d_out 16-byte aligned; the bytes between
 * the row's end and the next multiple of 16 are clobbered.  Unaligned mode: row_pitch must be >= the longest row
 * (reference length + total label bytes is always enough; see v2m_max_unaligned_length()).
 * row_lengths_out (host, optional, [n_rows]) receives each row's length.
 * The call returns once the kernels are QUEUED on the ctx's stream (the batch's small row tables travel through two
 * pinned staging areas used in turn, so consecutive calls do not wait for each other's kernels); the first >= 1 GiB
 * launch of a ctx also times both store flavours, synchronously.
 * With row_lengths_out in unaligned mode the call waits for the kernels.  Use v2m_ctx_synchronize() before reading d_out. */
int v2m_splice_rows_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_out, uint64_t row_pitch, uint64_t *row_lengths_out);

/* Device memory for row output (the d_out of v2m_splice_rows_device), chosen by measurement: on MI355X the write rate
 * the splice's store pattern reaches differs by up to ~25 % between hipMalloc'ed buffers, depending on how fragmented
 * their physical backing is, which a caller cannot see from a pointer.  Allocates up to `candidates` buffers of
 * `bytes` (fewer if HBM runs out -- all of them are held until the choice is made), times the store pattern on each,
 * keeps the fastest and frees the others; v2m_ctx_info() reports the rates.  candidates <= 1 (or a buffer too small to
 * probe) is a plain allocation.  Free with v2m_free_output().  Synchronous.
 * A side effect to know about: the driver wipes freed device memory that has been written, in the background, and while it
 * does (about 3 s per freed 63-GB candidate, measured) the process's device-to-host copies run at ~70 % of the link's rate
 * (profiles/r04/e2e_slow_after_alloc_output.txt).  A caller that is about to stream rows to the host (v2m_splice_rows) and
 * cares about those first seconds asks for one candidate. */
int v2m_alloc_output(v2m_ctx *ctx, uint64_t bytes, int candidates, void **d_out);
int v2m_free_output(v2m_ctx *ctx, void *d_ptr);
/* `bytes` bytes of device memory at d_src (a buffer of v2m_alloc_output, or any device memory of the context's device) to host memory
 * at dst, after everything queued on the context's stream: how a caller without a HIP runtime of its own reads what a device form
 * (v2m_diversity_of_counts, for one) left on the device.  bytes == 0 returns V2M_OK.  Synchronous. */
int v2m_read_output(v2m_ctx *ctx, const void *d_src, uint64_t bytes, void *dst);

/* Upper bound of any unaligned row's length for the uploaded graph (with a column window: the window's length). */
uint64_t v2m_max_unaligned_length(const v2m_ctx *ctx);

/* ---- column windows ---------------------------------------------------------------------------
 *
 * A column window [col_begin, col_end), 0 <= col_begin < col_end <= L = v2m_aligned_length(), makes every following
 * v2m_splice_rows, v2m_splice_rows_held and v2m_splice_rows_device call produce window bodies instead of whole rows:
 *   - aligned mode: bytes [col_begin, col_end) of the whole aligned row, exactly;
 *   - unaligned mode: every byte the walk emits sits in its own column (a reference segment or label never exceeds its aligned span,
 *     the padding fills the rest); the body is the emitted bytes whose column lies in the window, in order.  The walk's padding is
 *     left out, a '-' that is part of the reference or of a label is kept, so the body is never longer than col_end - col_begin;
 *   - V2M_SPLICE_BGZF: the members cover the window body, cut into 65 280-byte pieces from its first byte.
 * A window equal to the whole row gives exactly the bytes of no window.  Row order, cut semantics and everything else are unchanged;
 * v2m_aligned_length() stays L, while v2m_min_row_pitch(), v2m_max_unaligned_length() and the row_pitch rules of
 * v2m_splice_rows_device describe the window's rows.  The work of a row call scales with the window: its tiles and the edge words
 * that reach into it (plus the look-back of their restart points).
 * v2m_upload_graph resets the window to the whole row, and so does v2m_set_column_window(ctx, 0, L).  Returns V2M_ERR_STATE
 * before an upload and V2M_ERR_INVALID_ARGUMENT for an empty or out-of-range window.  Synchronous.
 * A reference range [s, e) (0-based, half-open) is the window [col(s), col(e)) with col(p) = aligned_positions[n] +
 * (p - reference_positions[n]) for the last node n with reference_positions[n] <= p, and col(reference length) = L. */
int v2m_set_column_window(v2m_ctx *ctx, uint64_t col_begin, uint64_t col_end);
/* col_end - col_begin of the window; L without one (0 before an upload). */
uint64_t v2m_window_length(const v2m_ctx *ctx);

/* ---- window sets ------------------------------------------------------------------------------
 *
 * A set of column windows is a third view beside whole rows and the column window: window k is [col_begin[k], col_end[k]) with
 * 0 <= col_begin[k] < col_end[k] <= L.  Windows may overlap, repeat and come in any order; order k is the caller's and is kept.
 * One row call splices every window of the set: a row's RECORD is record_pitch bytes, and piece k of it sits at slot_offset[k]:
 *   slot_offset[0] = 0, slot_offset[k + 1] = slot_offset[k] + (col_end[k] - col_begin[k] rounded up to 16),
 *   record_pitch = the end of the last slot rounded up to 256 (the v2m_min_row_pitch rule, applied to the record).
 * The 16 is that of the 16-byte row stores: every slot starts 16-byte aligned relative to its record.
 * Piece (row, k) is exactly the body that v2m_set_column_window(ctx, col_begin[k], col_end[k]) followed by a row call gives for
 * that row in the same mode (see "column windows": the aligned slice, the unaligned "emitted bytes whose column lies in the
 * window", founder rows with cuts, the REF row).  Its length lengths[k] is the window's length in aligned mode and the emitted
 * count (at most the window's length) in unaligned mode.
 * What a call may write into a record: aligned, bytes [slot_offset[k], slot_offset[k] + (length of window k rounded up to 16)) --
 * the tail of the last 16-byte chunk is clobbered; unaligned, bytes [slot_offset[k], slot_offset[k] + lengths[k]) and nothing else.
 * The set is independent of the column window: the set calls use it whatever v2m_set_column_window says, and v2m_splice_rows,
 * v2m_splice_rows_held and v2m_splice_rows_device never see it.  v2m_upload_graph drops it.  V2M_SPLICE_BGZF and a held form are
 * not available through the set calls (V2M_ERR_UNSUPPORTED).
 * Errors: V2M_ERR_STATE before an upload or when a splice call finds no set; V2M_ERR_INVALID_ARGUMENT for n_windows == 0 or an
 * empty or out-of-range window (the message names the window's index); V2M_ERR_UNSUPPORTED when the end of the last slot reaches
 * 2^32 or the tile count does not fit 32 bits (the unaligned kernels keep per-tile destinations in 32 bits); V2M_SPLICE_UNALIGNED
 * on a graph with a NUL byte refuses as the row calls do. */

/* The layout of a set (context-free, no device needed): slot_offset[n_windows] and *record_pitch.  Only begin < end is checked
 * here (the aligned length is a context's). */
int v2m_window_set_layout(uint64_t n_windows, const uint64_t *col_begin, const uint64_t *col_end,
                          uint64_t *slot_offset /* [n_windows] */, uint64_t *record_pitch);
/* Makes the windows the context's set (replacing an earlier one).  Synchronous. */
int v2m_set_window_set(v2m_ctx *ctx, uint64_t n_windows, const uint64_t *col_begin, const uint64_t *col_end);
uint64_t v2m_window_set_size(const v2m_ctx *ctx);      /* number of windows; 0 when none is set */
uint64_t v2m_window_set_pitch(const v2m_ctx *ctx);     /* record_pitch of the set; 0 when none is set */
/* One call per row, in row order: the row's record (piece k at record + slot_offset[k], lengths[k] bytes); both are the
 * library's and valid for the duration of the call. */
typedef int (*v2m_window_sink_fn)(void *user, uint64_t row_index, const char *record, const uint32_t *lengths /* [n_windows] */);
int v2m_splice_window_set(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_window_sink_fn sink, void *user);
/* Records into device memory: row r's record at d_out + r * record_pitch; record_pitch is any multiple of 16 that is at least
 * the end of the last slot.  d_out is 16-byte aligned. */
int v2m_splice_window_set_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_out, uint64_t record_pitch,
                                 uint32_t *lengths_out /* host, optional, [n_rows][n_windows] */);

/* ---- distinct pieces of a window set ------------------------------------------------------------
 *
 * Within a window most rows are byte-identical.  v2m_splice_window_set_distinct splices the set as v2m_splice_window_set does, but
 * the records stay in device memory: it finds the distinct pieces of every window there and reports each once, with the table of
 * which row has which.
 *   Equality.  Piece (r, k) is exactly the piece v2m_splice_window_set gives for that row, window and mode.  Two pieces of the same
 *     window are equal when they have the same length and the same bytes -- by bytes, not by path bits or effective edges: two
 *     different ALT records with the same label give equal pieces.
 *   Class numbering.  The classes of window k are numbered 0, 1, ... in the order of their first row in batch order.
 *     class_of_out[r * n_windows + k] is the class of piece (r, k); n_classes_out[k] the number of classes of window k.  Repeated or
 *     overlapping windows are independent windows.  All empty pieces of a window (unaligned mode) form one class of length 0.
 *   Sink.  `sink` is called once per class, on the calling thread, before the call returns: (user, window, class index, the class's
 *     first row, its bytes, their number).  Calls come in ascending first_row, and for equal first_row in ascending window.  `bytes`
 *     is library-owned pinned memory, valid during the call only.  A non-zero return ends the call with V2M_ERR_SINK.  With
 *     sink == NULL only the class tables are produced and no piece crosses the link.
 *   Errors.  V2M_SPLICE_BGZF (and a held form) is V2M_ERR_UNSUPPORTED.  As for v2m_splice_window_set: V2M_ERR_STATE without a graph
 *     or without a set, V2M_ERR_PRECONDITION for bad cuts, V2M_ERR_UNSUPPORTED for V2M_SPLICE_UNALIGNED on a graph with a NUL byte.
 *     A NULL class_of_out is V2M_ERR_INVALID_ARGUMENT.  n_rows == 0 returns V2M_OK with n_classes_out zeroed.
 *   State.  The column window, the set and every other call are untouched.
 *   Pool limit.  The distinct pieces of one call are kept in a device pool (each once, 16-byte aligned) until the call returns.  When
 *     they exceed V2M_DISTINCT_POOL_BYTES (environment, read per call; default 4 GiB; clamped to the free device memory) the call
 *     returns V2M_ERR_OUT_OF_MEMORY; the message names the knob and the bytes needed so far; the outputs are then unspecified.
 * How: the batch goes through the device in row slices (V2M_RING_SLOT_BYTES caps a slice's records plus tables, as elsewhere).  Per
 * slice hash_pieces_kernel gives every piece a 64-bit key -- the checksum of v2m_checksum_rows_device ("verification helper") of the
 * piece --, the host looks the keys up per (window, key, length), gather_pieces_kernel copies the pieces with unknown keys into the
 * pool as their classes' representatives, and verify_pieces_kernel compares every other piece with its candidate byte for byte.  A
 * mismatch is a key collision: the piece tries the next class with that key or becomes a representative in a further round, so the
 * result never depends on the key's quality (V2M_DISTINCT_HASH_BITS = 0 ... 64, a test knob read per call, keeps only that many low
 * bits of every key: the same classes after more rounds).  Synchronous. */
typedef int (*v2m_distinct_sink_fn)(void *user, uint64_t window, uint64_t class_index, uint64_t first_row, const char *bytes, uint64_t length);
int v2m_splice_window_set_distinct(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_SPLICE_UNALIGNED */,
                                   v2m_distinct_sink_fn sink /* may be NULL */, void *user,
                                   uint32_t *class_of_out /* host, [n_rows][n_windows] */,
                                   uint32_t *n_classes_out /* host, optional, [n_windows] */);

/* ---- row alignment ops --------------------------------------------------------------------------
 *
 * The coordinate map between a row and the reference, as run-length ops (what a chain or a CIGAR is made of).
 * For a row, every aligned column c in [0, L) has two facts:
 *   ref -- the REF row holds a reference byte there, not the walk's padding;
 *   row -- this row holds a reference or label byte there, not the walk's padding.
 * "Padding" is the walk's padding exactly as the unaligned mode defines it (sequence_writer.cc:80-83): a literal '-' inside the
 * reference or inside a label is a byte, not padding.  The column's class:
 *   ref and row -> M     row only -> I     ref only -> D     neither -> none (the column is skipped)
 * The row's ops are the run-length encoding of the classes of its non-skipped columns, in column order; skipped columns do not break
 * a run.  Op codes are BAM's: M = 0, I = 1, D = 2.  With flags = 0, M covers match and mismatch; V2M_OPS_SPLIT_MATCH (below) splits it
 * into BAM's '=' (7) and 'X' (8).
 * Guarantees: no op has length 0; no two neighbouring ops have the same code; the lengths of M and D sum to the reference length;
 * those of M and I to the row's unaligned length (what v2m_splice_rows_device reports for the row with V2M_SPLICE_UNALIGNED, passed
 * to the sink as row_length); the REF row (V2M_PLOIDY_MAX, no cuts) is the single op M R (no op for an empty reference); rows with
 * cuts follow the same rule on the row they would splice.
 * Rows arrive in batch order, one call per row, on the calling thread; `ops` is library-owned and valid during the call only; a
 * non-zero return ends the call with V2M_ERR_SINK.  Synchronous.  flags must be 0 or V2M_OPS_SPLIT_MATCH, anything else is
 * V2M_ERR_INVALID_ARGUMENT.  Errors as for v2m_splice_rows: V2M_ERR_STATE
 * before an upload, V2M_ERR_PRECONDITION for bad cuts; a graph with a NUL byte is refused as V2M_SPLICE_UNALIGNED refuses it.
 * The ops always describe the WHOLE row: a column window or window set in force is neither used nor disturbed.
 * A row's first op is never I: column 0 holds the first reference byte (node 0 sits at reference and aligned position 0), so its class is M or D.
 * The call works through the batch in slices of as many rows as keep the per-row tables of its first two passes (three words per tile
 * and the effective-edge words) within 256 MiB of device memory; a slice is counted once and its rows' records (12 bytes per op) come to
 * the host in pieces of consecutive rows that fit 64 MiB of device and of pinned memory each (V2M_OPS_SLICE_BYTES overrides the 64 MiB, a
 * test knob; a single row goes through whatever it takes).
 *
 * V2M_OPS_SPLIT_MATCH: every column of class M gets a further fact, eq.  The REF row's byte is the 0-padded template's byte at that
 * column, the row's byte the built row's byte there (a reference byte, or a label byte over it); eq holds when the two are equal AFTER
 * FOLDING ASCII LETTERS TO ONE CASE, and only those: bytes a and b are equal when a == b, or when (a ^ b) == 0x20 and (a | 0x20) lies
 * in 'a'..'z'.  So 'a' over 'A' is '=' (a soft-masked reference under an upper-case ALT is no mismatch); '@' / '`', '[' / '{' and
 * 0xC4 / 0xE4 are 'X'; 'N' over 'A' is 'X' (no IUPAC semantics); a literal '-' over a literal '-' is '='.  The column's class is then
 * '=' (V2M_OP_EQ), 'X' (V2M_OP_X), I, D or none, and the ops are the run-length encoding over the non-skipped columns exactly as above:
 * skipped columns do not break a run here either, and V2M_OP_M does not occur.  Guarantees: no op has length 0; no two neighbouring
 * ops have the same code; the lengths of =, X and D sum to the reference length, those of =, X and I to the row's unaligned length;
 * REPLACING 7 AND 8 BY 0 AND MERGING EQUAL NEIGHBOURS GIVES EXACTLY THE OPS OF flags = 0 FOR THE SAME ROW; the REF row is the single op
 * = R; rows with cuts follow the row they would splice.  Everything else above holds unchanged: whole rows only, windows and window
 * sets untouched, NUL bytes refused, the sink and error rules, the slices. */
typedef struct v2m_aln_op { uint32_t op; uint32_t length; } v2m_aln_op;
#define V2M_OP_M 0u
#define V2M_OP_I 1u
#define V2M_OP_D 2u
#define V2M_OP_EQ 7u
#define V2M_OP_X 8u
#define V2M_OPS_SPLIT_MATCH 0x4u
typedef int (*v2m_ops_sink_fn)(void *user, uint64_t row_index, const v2m_aln_op *ops, uint64_t n_ops, uint64_t row_length /* unaligned length */);
int v2m_row_ops(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_OPS_SPLIT_MATCH */, v2m_ops_sink_fn sink, void *user);

/* ---- column counts ------------------------------------------------------------------------------
 *
 * The alignment by column: for every column of the view, how many rows of the batch hold which base there.  The view is the whole row,
 * or the column window of v2m_set_column_window (a window set in force is ignored, as the row calls ignore it); it has
 * L = v2m_window_length() columns.  Only the aligned form exists: the flag bits 0x1, 0x2 and 0x4 are V2M_ERR_INVALID_ARGUMENT.
 * For column i of the view, count[c][i] is the number of batch rows whose aligned byte b at that column is of class c:
 *   c = 0 .. 3  A, C, G, T: (b | 0x20) == 'a', 'c', 'g', 't'.  Exactly the two ASCII letters match: 0x41 and 0x61 are A, 0xC1 and 0xE1 are not.
 *   c = 4       N: (b | 0x20) == 'n'
 *   c = 5       gap: b == '-' exactly (0x0D is no gap), whether the '-' is the walk's padding or a literal byte of the reference or of a
 *               label: the counts describe the bytes the A2M file holds
 *   c = 6       other: n_rows minus the sum of the six.  Derived, never stored.
 * Rows may repeat in a batch and every occurrence counts; a row with cuts counts as the row it splices.  n_rows < 2^32 - 1 as for every
 * row call, so no count overflows.  A column is VARIABLE when none of the seven classes holds all n_rows rows (a column where every row
 * is "other" is not variable; with n_rows <= 1 no column is).
 *
 * Device form.  d_counts is u32[V2M_COUNT_CLASSES][plane_pitch], 16-byte aligned; plane_pitch % 4 == 0 and plane_pitch >= (L + 3) & ~3.
 * Element i < L of plane c is overwritten with count[c][i] -- with V2M_COUNTS_ACCUMULATE it is added to; elements L ..< (L + 3) & ~3 are
 * written as 0, or left alone under V2M_COUNTS_ACCUMULATE; nothing beyond them is touched.
 * Sink form.  One record per column (flags = 0) or per variable column (V2M_COUNTS_VARIABLE_ONLY), in ascending column order; `column`
 * is absolute (the view's begin + i).  Records arrive in blocks of at most V2M_COLUMN_COUNTS_BLOCK_BYTES (environment, read per call;
 * default 64 MiB; a test knob like V2M_OPS_SLICE_BYTES), on the calling thread, in library-owned pinned memory valid during the call
 * only; the sink is never called with n = 0; a non-zero return ends the call with V2M_ERR_SINK.
 * Errors as for the row calls: V2M_ERR_INVALID_ARGUMENT for NULL pointers, unknown flags, a misaligned d_counts or a bad pitch,
 * V2M_ERR_STATE without a graph, V2M_ERR_PRECONDITION for bad cuts.  n_rows == 0 returns V2M_OK and touches nothing.  Both synchronous.
 * The column window and the window set are left as they were.
 * How: the batch goes through one device slot in row slices (as v2m_splice_window_set_distinct's does); per slice the aligned splice,
 * then column_counts_kernel adds the slice's rows into the table (d_counts, or a context-owned one of 6 * L * 4 bytes); a call of
 * many slices of few rows each (whole rows of a hundred million columns) carries the kernel's byte-wide counters from slice to slice in
 * a context-owned stage of 6 bytes per column and widens them into the table before they would pass 255 rows.  The sink form then selects per column range (count_variable_columns_kernel, scan_tile_counts_kernel, emit_column_counts_kernel), a range's
 * records crossing the link while the sink has the previous range's. */
#define V2M_COUNT_CLASSES 6
#define V2M_COUNTS_VARIABLE_ONLY 0x8u
#define V2M_COUNTS_ACCUMULATE    0x10u

typedef struct {
	uint64_t column;                      /* absolute aligned column */
	uint32_t count[V2M_COUNT_CLASSES];
} v2m_column_count;                       /* 32 bytes */

typedef int (*v2m_column_counts_sink_fn)(void *user, const v2m_column_count *cols, uint64_t n);

int v2m_column_counts(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_COUNTS_VARIABLE_ONLY */,
                      v2m_column_counts_sink_fn sink, void *user);

int v2m_column_counts_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_COUNTS_ACCUMULATE */,
                             void *d_counts, uint64_t plane_pitch);

/* ---- pair distances -----------------------------------------------------------------------------
 *
 * The alignment by pair of rows: an n_rows x n_rows matrix of how many columns of the view two rows of the batch differ in -- what
 * snp-dists prints, and what neighbour joining and clustering start from.  The view is that of the column counts: the whole row, or the
 * column window of v2m_set_column_window (a window set in force is ignored); L = v2m_window_length() columns.  The class of an aligned
 * byte is exactly the column counts' (above): 0-3 A, C, G, T; 4 N; 5 gap ('-' exactly); 6 other.
 *   flags = 0             dist[i][j] = the columns where the class of batch row i differs from that of batch row j.  All "other" bytes are
 *                         one class: 'R' against 'Y' counts as equal, and so does 'a' against 'A'.
 *   V2M_DIST_ACGT_ONLY    dist[i][j] = the columns where both classes are in 0-3 and differ (snp-dists' default).
 * Every other flag bit -- 0x1, 0x2, 0x4, 0x8 and 0x10 included -- is V2M_ERR_INVALID_ARGUMENT.
 * Rows may repeat: their distance is 0 and both entries exist; a row with cuts counts as the row it splices.  The matrix is symmetric
 * with a zero diagonal, and both triangles are written.  n_rows <= V2M_PAIR_DISTANCES_MAX_ROWS (32 768: 4 GiB of matrix); more rows, or
 * L >= 2^32, is V2M_ERR_UNSUPPORTED with a message that names the limit, before any device work.
 *
 * Device form.  d_dist is u32[n_rows][pitch], 16-byte aligned, pitch % 4 == 0 and pitch >= n_rows.  Elements [i][j < n_rows] are
 * overwritten (not added to); nothing else is touched.
 * Host form.  dist is u32[n_rows][n_rows] in host memory; the matrix is computed into a context-owned device buffer and copied.  info,
 * which may be NULL, receives n_sites (the VARIABLE columns of the view for this batch, as the column counts define them), n_columns
 * (L), n_passes, and -- while v2m_profile_enable is on, else 0 -- the times of the call's three stages in ms.  A stage's time is the
 * time elapsed on the context's stream between events around everything the stage queues (every slice's splice and kernel for the
 * counts and the pack stage), so it holds the gaps the host's queueing leaves between launches: it bounds the stage's kernel time from
 * above and is not a sum of kernel times.  That is how the stages are timed: they have no V2M_KERNEL_* ids, and V2M_KERNEL_LIMIT
 * keeps its value.
 * Errors as for the column counts: V2M_ERR_INVALID_ARGUMENT for NULL pointers, unknown flags, a misaligned d_dist or a bad pitch,
 * V2M_ERR_STATE without a graph, V2M_ERR_PRECONDITION for bad cuts.  n_rows == 0 returns V2M_OK and touches nothing (info included);
 * L == 0 writes zeros.  Both forms are synchronous.  The column window and the window set are left as they were, and so is what
 * v2m_column_counts returns afterwards.
 * How: a column where one class holds every row adds 0 to every pair under both definitions, so only the variable columns -- the
 * sites -- count.  (1) The column counts of the batch into the context's table, as v2m_column_counts makes them, and the selection
 * of the variable columns into a site list (emit_site_columns_kernel).  (2) A second pass over the same row slices: per slice the
 * aligned splice, then pack_sites_kernel gathers the rows' bytes at the sites into three bit planes of 3-bit class codes.  (3)
 * pair_distances_kernel: XOR + popcount over the planes, a workgroup a tile of 64 x 64 rows of the upper triangle (the mirror entry is
 * written too), the site words through LDS in chunks of 8; with few rows the site words are split over the grid and the parts meet
 * by integer atomicAdd on a zeroed matrix.  The planes take 3 * n_rows * n_sites / 8 bytes; V2M_PAIR_DISTANCES_PLANE_BYTES
 * (environment, read per call; default 16 GiB; a test knob like V2M_COLUMN_COUNTS_BLOCK_BYTES) bounds them: sites that do not fit
 * are taken in ranges of whole chunks, each range repeating (2) and (3) and adding into the matrix; n_passes counts the ranges.
 * V2M_PAIR_DISTANCES_PARTS (environment, read once per call; a test knob as well) overrides the number of parts the site words of a
 * launch of pair_distances_kernel are split into: the parts hold ceil(chunks / parts) chunks each and the last one the remainder. */
#define V2M_DIST_ACGT_ONLY 0x20u
#define V2M_PAIR_DISTANCES_MAX_ROWS 32768u

typedef struct {
	uint64_t n_sites;     /* variable columns of the view for this batch */
	uint64_t n_columns;   /* L */
	uint64_t n_passes;    /* site ranges the plane budget made (0 when there was no site) */
	double counts_ms;     /* column counts + site selection: stream time elapsed over the stage, see above */
	double pack_ms;       /* splices of the second pass + pack_sites_kernel: likewise */
	double pairs_ms;      /* pair_distances_kernel (with the zeroing of the matrix, where the parts meet by atomics) */
} v2m_pair_distances_info;    /* 48 bytes */

int v2m_pair_distances(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_DIST_ACGT_ONLY */,
                       uint32_t *dist /* n_rows x n_rows, host */, v2m_pair_distances_info *info /* may be NULL */);

int v2m_pair_distances_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_DIST_ACGT_ONLY */,
                              void *d_dist, uint64_t pitch);

/* ---- variable sites -----------------------------------------------------------------------------
 *
 * The alignment reduced to its variable columns: the rows of the batch, cut down to the selected columns of the view -- the FASTA
 * snp-sites makes from a multi-FASTA, and what IQ-TREE, RAxML, FastTree and Gubbins read.  The view is that of the column counts: the
 * whole row, or the column window of v2m_set_column_window (a window set in force is ignored); L = v2m_window_length() columns.  The
 * selection is decided from the column counts of the batch alone (classes as above: 0-3 A, C, G, T; 4 N; 5 gap; 6 other):
 *   flags = 0        the VARIABLE columns exactly as the column counts define them: none of the seven classes holds all n_rows rows.
 *                    These are the sites of v2m_pair_distances with flags 0 (its info's n_sites).
 *   V2M_SITES_SNP    the columns where at least two of the four classes A, C, G, T have a non-zero count (snp-sites' default rule):
 *                    exactly the columns that can add to a V2M_DIST_ACGT_ONLY distance.  Columns that vary only by gap, N or "other"
 *                    -- above all the padding columns of inserted ALT alleles -- are left out.
 * Every other flag bit -- 0x1, 0x2, 0x4, 0x8, 0x10 and 0x20 included -- is V2M_ERR_INVALID_ARGUMENT.  With n_rows <= 1 there is no
 * site.  The bytes delivered are the bytes the A2M file holds at those columns, unchanged: case, '-', 'N' and every other byte as they
 * are.  Rows may repeat; a row with cuts is the row it splices.  L >= 2^32 is V2M_ERR_UNSUPPORTED with a message that names the limit,
 * before any device work.  V is the number of selected columns.
 *
 * Device form.  d_bytes is u8[n_rows][pitch], 16-byte aligned, pitch % 16 == 0; d_columns, which may be NULL, is u32[pitch] and
 * receives the selected columns relative to the view, ascending; *n_sites receives V.  If V > pitch the call fails with
 * V2M_ERR_INVALID_ARGUMENT and a message that names V: *n_sites is set, nothing is written to either buffer, and the caller sizes its
 * buffers and calls again.  Otherwise bytes [r][s < V] and d_columns[s < V] are overwritten, bytes [r][V ..< (V + 3) & ~3] are
 * written as 0 (a lane stores whole words), and nothing else is touched.
 * Host form.  columns_sink is called once, before any row, with the ABSOLUTE aligned columns, ascending (as v2m_column_count.column
 * is absolute); rows_sink then receives blocks of consecutive batch rows in batch order: row first_row + r of the batch is the
 * n_sites bytes at bytes + r * pitch.  That memory is library-owned pinned memory, valid during the call only, on the calling thread.
 * Neither sink is ever called with zero sites or zero rows; a non-zero return stops the call with V2M_ERR_SINK; either may be NULL,
 * and a NULL sink's deliveries are skipped.  info, which may be NULL, receives n_sites (V), n_columns (L) and -- while
 * v2m_profile_enable is on, else 0 -- the stream time elapsed over the call's two stages in ms, timed as the pair distances' stages
 * are (above): no V2M_KERNEL_* ids, V2M_KERNEL_LIMIT keeps its value.
 * Errors as for the pair distances: V2M_ERR_INVALID_ARGUMENT for NULL rows or n_sites, unknown flags, a misaligned d_bytes or a bad
 * pitch, V2M_ERR_STATE without a graph, V2M_ERR_PRECONDITION for bad cuts.  n_rows == 0 returns V2M_OK and touches nothing (*n_sites
 * and info included).  Both forms are synchronous.  The column window and the window set are left as they were, and so is what
 * v2m_column_counts returns afterwards.
 * How: (1) the column counts of the batch into the context's table, as v2m_column_counts makes them, and the selection into a site
 * list: count_variable_columns_kernel / emit_site_columns_kernel for flags 0, count_snp_columns_kernel / emit_snp_columns_kernel for
 * V2M_SITES_SNP, scan_tile_counts_kernel between them.  (2) A second pass over the same row slices: per slice the aligned splice, then
 * gather_sites_kernel reads the rows' bytes at the sites -- a lane four sites, one 4-byte store per row -- into d_bytes (device form)
 * or into one of two context-owned buffers, from which the slice crosses the link on the copy stream into one of two pinned slots and
 * reaches rows_sink while the next slice is spliced and gathered. */
#define V2M_SITES_SNP 0x40u

typedef struct {
	uint64_t n_sites;     /* V: the selected columns of the view for this batch */
	uint64_t n_columns;   /* L */
	double counts_ms;     /* column counts + site selection: stream time elapsed over the stage */
	double gather_ms;     /* splices of the second pass + gather_sites_kernel: likewise, summed over the slices */
} v2m_variable_sites_info;    /* 32 bytes */

typedef int (*v2m_site_columns_sink_fn)(void *user, const uint64_t *columns, uint64_t n_sites);
typedef int (*v2m_site_rows_sink_fn)(void *user, uint64_t first_row, uint64_t n_rows, const char *bytes, uint64_t pitch, uint64_t n_sites);

int v2m_variable_sites(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_SITES_SNP */,
                       v2m_site_columns_sink_fn columns_sink /* may be NULL */, v2m_site_rows_sink_fn rows_sink /* may be NULL */, void *user,
                       v2m_variable_sites_info *info /* may be NULL */);

int v2m_variable_sites_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_SITES_SNP */,
                              void *d_columns /* may be NULL */, void *d_bytes, uint64_t pitch, uint64_t *n_sites);

/* ---- site LD ------------------------------------------------------------------------------------
 *
 * The alignment by pair of columns: linkage disequilibrium between nearby biallelic sites of the batch's rows, the four integer counts
 * that r^2 is made of, as plink --r2 reports it for phased haplotypes.  The view is that of the column counts: the whole row, or the
 * column window of v2m_set_column_window (a window set in force is ignored); L = v2m_window_length() columns.  Classes as above: 0-3 A,
 * C, G, T; 4 N; 5 gap; 6 other.
 * Sites.  Decided from the column counts of the batch alone: a column is a site when exactly two of the classes A, C, G, T have a
 * non-zero count and both counts are >= min_allele_count (>= 1).  lo < hi are those two classes.  At a site a row is CALLED when its
 * class is lo or hi and CARRIES when it is hi; rows of any other class (N, gap, other; case is ignored as the classes ignore it) are
 * missing there.  V is the number of sites, ascending by column; with n_rows <= 1, V = 0.
 * Pairs.  (s, t), site indices with s < t, t - s <= window_sites (1 ... V2M_SITE_LD_MAX_WINDOW) and, unless window_columns is 0,
 * column[t] - column[s] <= window_columns: the candidates.  Over the batch rows (a repeated row counts every time; a row with cuts is the
 * row it splices):
 *   n      rows called at both sites          n_a    rows called at both that carry at s
 *   n_ab   rows that carry at both            n_b    rows called at both that carry at t
 * D = n n_ab - n_a n_b and den = n_a (n - n_a) n_b (n - n_b).  A pair is REPORTED iff den != 0 and D^2 min_r2_den >= min_r2_num den:
 * compared exactly in integers (n_rows <= V2M_SITE_LD_MAX_ROWS = 32 768 keeps D^2 and den inside 64 bits; the two products are taken
 * 128 bits wide), never in floating point; 1 <= min_r2_den <= 1 000 000 and 0 <= min_r2_num <= min_r2_den.  Reported pairs are
 * delivered ascending by (s, t).  r^2 = D^2 / den as a floating-point number appears only where a caller prints it.
 *
 * Host form.  sites_sink is called once with all V site records, before any pair.  pairs_sink then receives blocks of reported pairs in
 * order.  Both get library-owned pinned memory valid during the call only, and neither is ever called with n = 0.  Either sink may be NULL; a
 * non-zero return is V2M_ERR_SINK.  info, which may be NULL, receives V, L, the reported pairs, the candidates, and -- while
 * v2m_profile_enable is on, else 0 -- the stream time elapsed over the three stages, timed as the pair distances' stages are.
 * Device form.  d_sites (v2m_ld_site[site_capacity]) and d_pairs (v2m_ld_pair[pair_capacity]) are 16-byte aligned; d_pairs may be
 * NULL with pair_capacity 0, to ask for the counts only (then nothing is written to either buffer unless the call succeeds, which it
 * does only when no pair is reported).  *n_sites and *n_pairs receive V and the number of reported pairs.  When V > site_capacity or
 * the reported pairs exceed pair_capacity the call fails with V2M_ERR_INVALID_ARGUMENT, a message that names both numbers, both
 * outputs set and nothing written; otherwise exactly records [0, V) and [0, n_pairs) are written.
 * Errors, worded and ordered as for v2m_variable_sites: V2M_ERR_INVALID_ARGUMENT for NULL rows or params, parameters out of range, NULL
 * outputs or misaligned buffers; V2M_ERR_UNSUPPORTED, with a message that names the limit, for more rows than V2M_SITE_LD_MAX_ROWS,
 * L >= 2^32 (both before any device work) or planes beyond the budget (below; before any device work beyond the counts);
 * V2M_ERR_STATE without a graph; V2M_ERR_PRECONDITION for bad cuts.  n_rows == 0 returns V2M_OK and touches nothing.  Both forms are
 * synchronous.  The column window and the window set are left as they were, and so is what v2m_column_counts returns afterwards.
 * How (csrc/ld_kernels.hpp).  (1) The column counts into the context's table; count_ld_columns_kernel / scan_tile_counts_kernel /
 * emit_ld_columns_kernel make the site list and the records.  (2) A second pass over the row slices: per slice the aligned splice, then
 * ld_pack_kernel ORs the rows' called and carries bits into two bit planes by site over rows, u64[row word][2][V rounded up to 64],
 * 16 * V_pad * ceil(n_rows / 64) bytes.  V2M_SITE_LD_PLANE_BYTES (environment, read per call; default 16 GiB) bounds them: beyond it
 * the call is V2M_ERR_UNSUPPORTED with the bytes needed in the message.  (3) ld_pairs_kernel<false>, a workgroup a tile of 64 x 64
 * sites of the band, AND + popcount with the row words through LDS, counts the reported pairs per (site, tile);
 * scan_tile_counts_kernel turns the counts of a strip of 64 sites into offsets; ld_pairs_kernel<true> computes the tiles that hold a
 * pair again and writes every pair at its rank: the order (s, t) with no sort.  The host form emits ranges of whole strips whose
 * records fit V2M_SITE_LD_BLOCK_BYTES (environment, read per call; default 64 MiB, at least one strip) into two buffers in turn; a
 * range crosses the link on the copy stream while the next is emitted.  No V2M_KERNEL_* ids: V2M_KERNEL_LIMIT keeps its value. */
#define V2M_SITE_LD_MAX_WINDOW 4096u
#define V2M_SITE_LD_MAX_ROWS 32768u

typedef struct {
	uint32_t window_sites;       /* 1 ... V2M_SITE_LD_MAX_WINDOW */
	uint32_t min_allele_count;   /* >= 1 */
	uint32_t min_r2_num;         /* 0 ... min_r2_den */
	uint32_t min_r2_den;         /* 1 ... 1 000 000 */
	uint64_t window_columns;     /* 0: no limit */
} v2m_site_ld_params;    /* 24 bytes */

typedef struct {
	uint64_t column;             /* absolute aligned column */
	uint32_t class_lo, class_hi; /* the two classes, lo < hi, of 0-3 */
	uint32_t count_lo, count_hi; /* their counts over the batch */
} v2m_ld_site;           /* 24 bytes */

typedef struct {
	uint32_t site_a, site_b;     /* s < t: indices into the site records */
	uint32_t n, n_a, n_b, n_ab;
} v2m_ld_pair;           /* 24 bytes */

typedef struct {
	uint64_t n_sites;     /* V */
	uint64_t n_columns;   /* L */
	uint64_t n_pairs;     /* reported pairs */
	uint64_t n_candidates;/* pairs that satisfy the two window limits */
	double counts_ms;     /* column counts + site selection: stream time elapsed over the stage */
	double pack_ms;       /* splices of the second pass + ld_pack_kernel */
	double pairs_ms;      /* ld_pairs_kernel<false>, the scan, ld_pairs_kernel<true> */
} v2m_site_ld_info;      /* 56 bytes */

typedef int (*v2m_ld_sites_sink_fn)(void *user, const v2m_ld_site *sites, uint64_t n);
typedef int (*v2m_ld_pairs_sink_fn)(void *user, const v2m_ld_pair *pairs, uint64_t n);

int v2m_site_ld(v2m_ctx *ctx, const v2m_row_batch *rows, const v2m_site_ld_params *params,
                v2m_ld_sites_sink_fn sites_sink /* may be NULL */, v2m_ld_pairs_sink_fn pairs_sink /* may be NULL */, void *user,
                v2m_site_ld_info *info /* may be NULL */);

int v2m_site_ld_device(v2m_ctx *ctx, const v2m_row_batch *rows, const v2m_site_ld_params *params,
                       void *d_sites, uint64_t site_capacity, void *d_pairs /* may be NULL with capacity 0 */, uint64_t pair_capacity,
                       uint64_t *n_sites, uint64_t *n_pairs);

/* ---- neighbour joining --------------------------------------------------------------------------
 *
 * The tree of the batch's rows: canonical neighbour joining (Saitou & Nei 1987; Studier & Keppler 1988) on the matrix of the pair
 * distances, computed where the matrix lies.  This is the library's one floating-point result, and it is defined operation by
 * operation so that it has exactly one value: all arithmetic is IEEE binary64, round to nearest, every operation rounded on its own
 * and NEVER contracted into a fused multiply-add.
 *
 * Input and node ids.  n >= 3 taxa and the upper triangle d[i][j], i < j, of a u32 matrix; only those elements are read.  Leaves have
 * ids 0 ... n - 1; the node made at join t (t = 0 ...) has id n + t.  D(a, b) = (double) d to begin with, and R(a) = sum over b of
 * D(a, b): exact integers below 2^53, so that any order of summation gives the same value -- here, and only here.
 *
 * One join, repeated while r > 3 taxa remain:
 *   1. Q(a, b) = (double) (r - 2) * D(a, b) - (R(a) + R(b)): one product, one sum, one difference.
 *   2. The pair with the smallest Q; among equal Q the smallest lower id, then the smallest higher id (by id, never by where a taxon
 *      happens to lie in memory).  a is the lower id, b the higher.
 *   3. delta = (R(a) - R(b)) / (double) (r - 2);  len_a = 0.5 * (D(a, b) + delta);  len_b = D(a, b) - len_a.  Negative lengths are
 *      kept, as canonical NJ does.
 *   4. For every other live k: s = D(a, k) + D(b, k);  D(u, k) = 0.5 * (s - D(a, b));  R(k) = (R(k) - s) + D(u, k).
 *   5. R(u) = 0.5 * ((R(a) + R(b)) - (double) r * D(a, b)): the closed form, not a sum over k, so that no order of reduction enters.
 * The last three taxa a < b < c by id:
 *   len_a = 0.5 * ((D(a, b) + D(a, c)) - D(b, c));  len_b = 0.5 * ((D(a, b) + D(b, c)) - D(a, c));
 *   len_c = 0.5 * ((D(a, c) + D(b, c)) - D(a, b)).
 *
 * Result: n - 2 records.  Records 0 ... n - 4 are the joins in order, with c = V2M_NJ_NONE, len_c = 0 and reserved = 0; the last
 * record is the trifurcation.
 *
 * v2m_nj_tree_of_distances: d_dist is u32[n][pitch] in device memory, 16-byte aligned, pitch % 4 == 0 and pitch >= n, as
 * v2m_pair_distances_device writes it; it is not modified, and no graph is needed.  v2m_nj_tree: the distances of the batch over the
 * view in force (flags: 0 or V2M_DIST_ACGT_ONLY, as for the pair distances) go into a context-owned matrix and the tree is built from
 * it; the column window, the window set and what v2m_column_counts returns afterwards are left as they were.  nodes is host memory
 * for n - 2 records.  info, which may be NULL, receives n_nodes (n - 2), the pair distances' n_sites, n_columns and n_passes (0 for
 * v2m_nj_tree_of_distances) and -- while v2m_profile_enable is on, else 0 -- the stream time of the two stages in ms, as the pair
 * distances define it.  The kernels have no V2M_KERNEL_* ids.
 * n == 0 returns V2M_OK and touches nothing (info included); n == 1 and n == 2 are V2M_ERR_INVALID_ARGUMENT (there is no tree), and so
 * are NULL pointers, unknown flags, a misaligned d_dist and a bad pitch; n > V2M_NJ_MAX_ROWS (32 768: 8.6 GB of working matrix) is
 * V2M_ERR_UNSUPPORTED before any device work.  Rows may repeat (distance 0).  Both calls are synchronous.
 * How (csrc/nj_kernels.hpp): nj_init_kernel makes the working matrix double[n][n], R and the table of ids; then per join
 * nj_rowmin_kernel (a wave a row: the row's best (Q, lower id, higher id) over the live taxa, which lie dense in slots 0 ... r - 1)
 * and nj_join_kernel (one workgroup: the step's pair, the record, D(u, .) and the R updates; u takes one of the two slots and the last
 * live slot moves into the other); nj_last_kernel writes the trifurcation.  The host sizes every grid from r = n - t and queues all
 * 2 (n - 3) + 2 launches on the context's stream without a synchronisation in between; the records come back in one copy. */
#define V2M_NJ_NONE 0xFFFFFFFFu
#define V2M_NJ_MAX_ROWS 32768u

typedef struct {
	uint32_t a, b, c, reserved;     /* the joined ids, a < b (< c); c = V2M_NJ_NONE but in the last record */
	double len_a, len_b, len_c;     /* the branch from the new node to a, b (and c; 0 but in the last record) */
} v2m_nj_node;           /* 40 bytes */

typedef struct {
	uint64_t n_nodes;     /* records written: n - 2 */
	uint64_t n_sites;     /* of the pair distances (v2m_nj_tree) */
	uint64_t n_columns;   /* likewise: L */
	uint64_t n_passes;    /* likewise */
	double distances_ms;  /* the pair distances' three stages together: stream time, see "pair distances" */
	double tree_ms;       /* nj_init_kernel ... nj_last_kernel: likewise */
} v2m_nj_tree_info;      /* 48 bytes */

int v2m_nj_tree_of_distances(v2m_ctx *ctx, const void *d_dist, uint64_t n, uint64_t pitch, v2m_nj_node *nodes /* host, n - 2 */,
                             v2m_nj_tree_info *info /* may be NULL */);

int v2m_nj_tree(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_DIST_ACGT_ONLY */, v2m_nj_node *nodes /* host, n_rows - 2 */,
                v2m_nj_tree_info *info /* may be NULL */);

/* ---- bootstrap ----------------------------------------------------------------------------------
 *
 * Felsenstein's bootstrap of the neighbour-joining tree: the columns of the view are resampled with replacement, the tree is built
 * again from every replicate's distances, and each join of the real tree is given the number of replicate trees that hold its split.
 * The view, the seven classes, flags (0 or V2M_DIST_ACGT_ONLY), the row limits and the L < 2^32 limit are those of the pair
 * distances.  differ(i, j, c) is what column c of the view adds to dist[i][j] there: 0 or 1.
 *
 * Weighted distances.  For weights w[c], one u32 per column of the view: dist_w[i][j] = sum over c of w[c] * differ(i, j, c).  The sum
 * of w[c] over ALL columns of the view must be below 2^32 -- checked on the host before any device work, else
 * V2M_ERR_INVALID_ARGUMENT --, so that no entry can overflow a u32.  All-ones weights give the pair distances, all-zero weights give
 * zeros.  A column that is no site may carry any weight: it counts toward the sum rule and adds nothing else.
 *
 * The draws.  All arithmetic is mod 2^64.  G = 0x9E3779B97F4A7C15.  mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9, then
 * z = (z ^ (z >> 27)) * 0x94D049BB133111EB, then z ^ (z >> 31) (splitmix64's finaliser).  key = mix(seed + G).  Draw k (0 <= k < L) of
 * replicate r (a u32) is x = mix(key + ((r << 32 | k) + 1) * G) and selects column floor(x * L / 2^64): the high half of the 128-bit
 * product.  Replicate r's weight of column c is the number of its L draws that selected c; the weights sum to L, so the sum rule
 * always holds.  This is the bootstrap over the columns of the view, as seqboot does it, not a resampling of the variable sites only
 * (that the implementation looks at the sites alone is its own business).
 *
 * Replicate tree r: the tree v2m_nj_tree_of_distances builds from replicate r's weighted matrix, with the same arithmetic and ties.
 *
 * Support.  Join record t (0 <= t <= n - 4) of the main tree creates node n + t; the leaves under that node and the remaining leaves
 * are the split of the record.  The n - 3 splits of a tree are distinct and non-trivial.  Two splits are equal when they are the same
 * partition of the leaves into two sets, whichever side the node lies on and in whatever order the joins came.  support[t] is the
 * number of replicates 0 ... B - 1 whose tree holds the split of record t.  The trifurcation record has none; with n == 3 the array
 * is empty.
 *
 * v2m_pair_distances_weighted: weights is host memory, one u32 per column of the view (it may be NULL when L == 0); dist and info as
 * for v2m_pair_distances.  v2m_bootstrap_distances: replicate `replicate`'s weighted matrix, for any u32 replicate number.
 * v2m_nj_bootstrap: nodes (n - 2) receives the main tree, equal to v2m_nj_tree's; support (n - 3; may be NULL only when n == 3) the
 * counts; replicate_nodes, when not NULL, the n_replicates x (n - 2) records of the replicate trees.  1 <= n_replicates <=
 * V2M_NJ_BOOTSTRAP_MAX_REPLICATES and n >= 3, else V2M_ERR_INVALID_ARGUMENT in v2m_nj_tree's words; n == 0 returns V2M_OK and touches
 * nothing.  The other errors are those of the pair distances and of v2m_nj_tree, each before any device work.  With no site (V == 0
 * or L == 0) every matrix is zero, the trees are those of the zero matrix and every support is n_replicates.
 * All three calls are synchronous and leave the column window, the window set and what v2m_column_counts returns as they were.
 *
 * How (csrc/bootstrap_kernels.hpp, csrc/nj_support.hpp).  The counts, the site list and the bit planes are the pair distances'.  A
 * replicate's weights are kept by site rank, u32 w[V]: bootstrap_weights_kernel makes the L draws, finds each column in the site
 * list by bisection and adds the hits with integer atomicAdd (explicit weights: a gather).  weight_slices_kernel cuts w into 32 bit
 * slices laid out as a plane is and ORs all weights into one word, from which the host -- one 4-byte copy and one synchronisation a
 * replicate -- takes K, the bit length of the largest weight.  pair_distances_weighted_kernel<acgt_only> is pair_distances_kernel with
 * acc += sum over b < K of popcount(m & slice[b][word]) << b; K == 0 writes zeros and launches nothing.  When the planes fit
 * V2M_PAIR_DISTANCES_PLANE_BYTES they are packed ONCE and stay resident across the main matrix and every replicate
 * (n_pack_passes = n_passes = 1); otherwise every replicate runs the passes over again, the main matrix sharing those of
 * replicate 0 (n_pack_passes = n_replicates * n_passes for v2m_nj_bootstrap).  V2M_PAIR_DISTANCES_PARTS acts as on the plain path.  The splits are counted on the host, exactly. */
#define V2M_NJ_BOOTSTRAP_MAX_REPLICATES 100000u

typedef struct {
	uint64_t n_rows;          /* n */
	uint64_t n_sites;         /* of the pair distances */
	uint64_t n_columns;       /* L */
	uint64_t n_passes;        /* site ranges of one matrix (0 when there was no site) */
	uint64_t n_pack_passes;   /* times a range of planes was packed over the whole call */
	uint64_t n_replicates;    /* B */
	uint64_t max_slices;      /* the largest K of any replicate */
	double distances_ms;      /* the main matrix: counts, pack and pairs (stream time, see "pair distances") */
	double weights_ms;        /* all replicates: draws (or gather) and slices */
	double pairs_ms;          /* all replicates: pair_distances_weighted_kernel, with the zeroing and any repeated pack */
	double trees_ms;          /* the main tree and all replicate trees */
} v2m_nj_bootstrap_info;     /* 88 bytes */

int v2m_pair_distances_weighted(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_DIST_ACGT_ONLY */,
                                const uint32_t *weights /* host, one per column of the view */, uint32_t *dist /* n_rows x n_rows, host */,
                                v2m_pair_distances_info *info /* may be NULL */);

int v2m_bootstrap_distances(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_DIST_ACGT_ONLY */, uint64_t seed, uint32_t replicate,
                            uint32_t *dist /* n_rows x n_rows, host */, v2m_pair_distances_info *info /* may be NULL */);

int v2m_nj_bootstrap(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_DIST_ACGT_ONLY */, uint32_t n_replicates, uint64_t seed,
                     v2m_nj_node *nodes /* host, n_rows - 2 */, uint32_t *support /* host, n_rows - 3 */,
                     v2m_nj_node *replicate_nodes /* NULL, or host, n_replicates x (n_rows - 2) */, v2m_nj_bootstrap_info *info /* may be NULL */);

/* ---- parsimony ----------------------------------------------------------------------------------
 *
 * What changed where on a tree of the batch's rows: Fitch's parsimony (Fitch 1971) of every SNP site on the join records of a tree,
 * in integers throughout, so that every result has exactly one value.
 *
 * Tree.  n >= 3 leaves 0 ... n - 1 and n - 2 records of v2m_nj_node, as v2m_nj_tree writes them; any records that form a tree are
 * taken, they need not come from neighbour joining.  Record t makes node n + t from children with smaller ids, a < b (< c); only the
 * last record has a c; every id 0 ... 2 n - 4 is a child exactly once.  Anything else is V2M_ERR_INVALID_ARGUMENT, decided on the host
 * before any device work.  The lengths are ignored.  The root is the last node, 2 n - 3; every other node x has one branch, to its
 * parent.
 *
 * States.  A leaf's set at a site is a 4-bit mask: 1 << class for the column counts' classes 0-3 (A, C, G, T, either case), and 0xF
 * -- missing, compatible with anything -- for every other byte (N, gap, other, and the 0 padding of the gather).
 *
 * Up, per site, the records in order: X = S(a) & S(b); when that is empty, X = S(a) | S(b) and steps += 1.  The last record only:
 * Y = X & S(c); when Y is empty, steps += 1 and X stays, else X = Y.  S(n + t) = X.  present = the OR of the masks of the leaves
 * that are not missing.
 * Down, per site: state(root) = the lowest set bit of S(root).  Then the records from the last to the first, within a record the
 * children in the order a, b, c: state(x) = state(parent) when that bit is in S(x), else the lowest set bit of S(x).  Where state(x)
 * differs from the parent's, that is one mutation (site, x, from, to), from and to as classes 0-3.  A missing leaf never carries one.
 *
 * Results.  Per site, steps and present.  Per node x < 2 n - 3, branch_changes[x]: the mutations on its branch, summed over the
 * sites.  The mutations, ascending by site and within a site in the order of the down pass.  The mutations of a site number exactly
 * its steps, which is the least number of changes any assignment of states needs; the sum of branch_changes is the sum of steps.
 * steps does not depend on which node is the root; the mutations' branches and directions do: they are those of the root 2 n - 3.
 *
 * v2m_parsimony_of_sites (device form): d_bytes is u8[n][pitch] in device memory as v2m_variable_sites_device writes it, 16-byte
 * aligned with pitch % 16 == 0 and pitch >= V; only the first V bytes of a row count, and nothing is modified.  No graph is needed.
 * nodes is host memory.  d_sites (v2m_parsimony_site[V]), d_branch_changes (u32[2 n - 3]) and d_mutations (v2m_tree_mutation[capacity];
 * may be NULL with capacity 0, to ask for everything but the list) are device memory, 16-byte aligned.  *n_mutations is always set
 * when the passes ran.  When the mutations exceed a capacity that is not 0 the call fails with V2M_ERR_INVALID_ARGUMENT and a message
 * that names their number; d_sites is written, the list and d_branch_changes are not.  The sets are context-owned: (n - 2) * pitch bytes.
 * v2m_tree_parsimony (host form): the sites are those of v2m_variable_sites with V2M_SITES_SNP over the view in force -- no other
 * column can have steps > 0 -- for the rows of the batch as the leaves, row r leaf r.  flags is 0.  The sites are cut into ranges
 * that start at multiples of 256 sites and whose leaf bytes and sets, 2 n - 2 bytes a site, fit V2M_PARSIMONY_BYTES (environment,
 * read per call; default 16 GiB, at least 256 sites); per range the second pass of the variable sites over the row slices, the two
 * passes above, and the range's records and mutations on their way to the host on the copy stream while the next range runs.
 * branch_changes (host, 2 n - 3; may be NULL) accumulates over the ranges.  sites_sink is called once with all V records (column
 * absolute), after the last range; mutations_sink receives blocks of mutations in order, site indices into those V records.  Both
 * get memory valid during the call only, neither is ever called with n = 0, either may be NULL; a non-zero return is V2M_ERR_SINK.
 * info, which may be NULL, receives V, L, the mutations (the tree's length), the ranges and -- while v2m_profile_enable is on, else
 * 0 -- the stream time of the three stages.  With V == 0 every branch count is 0 and no sink is called.
 * Limits and errors, worded and ordered as for v2m_variable_sites and v2m_nj_tree: n == 0 returns V2M_OK and touches nothing; n == 1
 * and n == 2 are V2M_ERR_INVALID_ARGUMENT; n > V2M_NJ_MAX_ROWS, V >= 2^32 and a call whose mutations reach 2^32 (the number is in the
 * message) are V2M_ERR_UNSUPPORTED.  Both calls are synchronous; the column window, the window set and what v2m_column_counts
 * returns afterwards are left as they were.
 * How (csrc/parsimony_kernels.hpp).  A lane owns four adjacent sites for the whole tree, a mask per byte of one u32, and the rule
 * above is a few byte-parallel operations on it.  fitch_up_kernel walks the records, classifies leaf bytes in flight, writes the
 * sets, the site records and its workgroup's steps; scan_tile_counts_kernel turns those into offsets; fitch_down_kernel<false> walks
 * the records backwards, writes states over the sets and adds every branch's changes with one integer atomicAdd per wave;
 * fitch_down_kernel<true> also writes each mutation at its site's offset plus its rank: the order above with no sort.  No
 * V2M_KERNEL_* ids: V2M_KERNEL_LIMIT keeps its value. */
typedef struct { uint32_t steps, present; } v2m_parsimony_site;               /* 8 bytes: device form */
typedef struct { uint64_t column; uint32_t steps, present; } v2m_tree_site;   /* 16 bytes: host form, column absolute */
typedef struct { uint32_t site, node, from, to; } v2m_tree_mutation;          /* 16 bytes */

typedef struct {
	uint64_t n_sites;      /* V: the SNP columns of the view for this batch */
	uint64_t n_columns;    /* L */
	uint64_t n_mutations;  /* the tree's length: the sum of steps */
	uint64_t n_ranges;     /* site ranges (0 when there was no site) */
	double counts_ms;      /* column counts + site selection: stream time elapsed over the stage */
	double gather_ms;      /* splices of the second pass + gather_sites_kernel, summed over the ranges */
	double parsimony_ms;   /* fitch_up_kernel, the scan, fitch_down_kernel: likewise */
} v2m_tree_parsimony_info;    /* 56 bytes */

typedef int (*v2m_tree_sites_sink_fn)(void *user, const v2m_tree_site *sites, uint64_t n);
typedef int (*v2m_tree_mutations_sink_fn)(void *user, const v2m_tree_mutation *mutations, uint64_t n);

int v2m_parsimony_of_sites(v2m_ctx *ctx, const void *d_bytes, uint64_t n, uint64_t n_sites, uint64_t pitch, const v2m_nj_node *nodes /* host, n - 2 */,
                           void *d_sites, void *d_branch_changes /* u32[2 n - 3] */, void *d_mutations /* may be NULL with capacity 0 */, uint64_t capacity,
                           uint64_t *n_mutations);

int v2m_tree_parsimony(v2m_ctx *ctx, const v2m_row_batch *rows, const v2m_nj_node *nodes /* host, n_rows - 2 */, uint32_t flags /* 0 */,
                       uint32_t *branch_changes /* host, 2 n_rows - 3, or NULL */, v2m_tree_sites_sink_fn sites_sink /* may be NULL */,
                       v2m_tree_mutations_sink_fn mutations_sink /* may be NULL */, void *user, v2m_tree_parsimony_info *info /* may be NULL */);

/* ---- window diversity ---------------------------------------------------------------------------
 *
 * The alignment summarised along the reference: per bin of columns the sums that nucleotide diversity, Watterson's theta, Tajima's D,
 * d_xy and F_ST are made of, and the folded site frequency spectrum -- all of them sums over columns of small integer functions of
 * the column counts (above), so every result is an integer with exactly one value, and the doubles are derived from them on the host.
 *
 * Per column.  A counts table is what v2m_column_counts_device writes, u32[V2M_COUNT_CLASSES][plane_pitch], counted over n rows; the
 * classes are the column counts'.  For column i let a, c, g, t be planes 0-3 and m = a + c + g + t; planes 4 and 5 (N, gap) are never
 * read.  All arithmetic is in u64.
 *   diffs(i)        = a c + a g + a t + c g + c t + g t: the pairs of batch rows that both hold A, C, G or T and differ.  Rows that
 *                     repeat count as the rows they are, as in the pair distances: summed over a view, diffs is the sum of the upper
 *                     triangle of v2m_pair_distances(..., V2M_DIST_ACGT_ONLY) over the same view.
 *   pairs(i)        = m (m - 1) / 2
 *   called(i)       : m >= 2
 *   segregating(i)  : at least two of a, c, g, t are non-zero
 *   complete(i)     : m == n and n >= 2
 * Between two tables over n_a and n_b rows (the same L and pitch), with m_A, m_B the two m:
 *   diffs(i)        = m_A m_B - (a_A a_B + c_A c_B + g_A g_B + t_A t_B)
 *   pairs(i)        = m_A m_B
 *   called(i)       : m_A >= 1 and m_B >= 1
 *
 * Bins.  bounds is u64[n_bins + 1], ascending but not strictly so; bin k is the columns [bounds[k], bounds[k + 1]), an empty bin is
 * legal, and columns before bounds[0] or from bounds[n_bins] on belong to no bin.  Bin k's record is v2m_diversity_bin (within) or
 * v2m_diversity_between_bin (between): `columns` = bounds[k + 1] - bounds[k], the counts of the columns that are called, segregating,
 * complete, complete and segregating, and the sums of diffs and pairs over the bin's columns and of diffs over its complete columns.
 *
 * Folded spectrum (within form only): sfs is u64[n / 2 + 1] over the columns of [bounds[0], bounds[n_bins]).  A complete column with
 * exactly one non-zero letter adds 1 to sfs[0]; with exactly two, 1 to sfs[the smaller of the two counts]; with three or four, 1 to
 * info->multiallelic.  Without a spectrum (sfs NULL) multiallelic is 0.
 *
 * Limits.  n, n_b <= V2M_DIVERSITY_MAX_ROWS (32 768, the limit of the pair distances) and L < 2^32: then no sum passes 2^62.  More rows, a
 * longer view, or 2^32 - 1 bins and more is V2M_ERR_UNSUPPORTED with a message that names the limit, before any device work.
 *
 * The doubles.  IEEE double, only + - * / and sqrt, each operation rounded on its own (no fused multiply-add, no libm call), integers
 * converted to double exactly (all are below 2^62, but only values below 2^53 convert without rounding: a conversion is one rounding
 * like any operation), in exactly this order.  d(x) is the conversion of the integer x.  A value whose denominator is zero does not
 * exist; the text writers print NA.  From a window's record (bins summed field by field as integers) and n:
 *   pi       = d(diffs) / d(pairs)                                    exists when pairs > 0
 *   a1       = 0; for i = 1 .. n - 1 ascending: a1 = a1 + 1 / d(i)
 *   a2       = 0; for i = 1 .. n - 1 ascending: a2 = a2 + 1 / (d(i) * d(i))
 *   S        = d(complete_segregating)
 *   theta_w  = S / a1                                                 exists when n >= 2
 *   b1       = (d(n) + 1) / (3 * (d(n) - 1))
 *   b2       = (2 * (d(n) * d(n) + d(n) + 3)) / (9 * d(n) * (d(n) - 1))            [9 * d(n) first, then * (d(n) - 1)]
 *   c1       = b1 - 1 / a1
 *   c2       = (b2 - (d(n) + 2) / (a1 * d(n))) + a2 / (a1 * a1)
 *   e1       = c1 / a1
 *   e2       = c2 / (a1 * a1 + a2)
 *   k        = d(complete_diffs) / (d(n) * (d(n) - 1) / 2)             [d(n) * (d(n) - 1) first, then / 2]
 *   v        = e1 * S + (e2 * S) * (S - 1)
 *   tajima_d = (k - S / a1) / sqrt(v)                                 exists when n >= 2 and v > 0
 *   dxy      = d(diffs) / d(pairs) of a between record                exists when pairs > 0
 *   fst      = 1 - (pi_A + pi_B) / (2 * dxy)                           Hudson's; exists when pi_A, pi_B and dxy exist and dxy > 0
 * Sums and products of more than two terms are evaluated left to right.  (n = 10, S = 16, k = 3.888889: a1 = 2.8289682539682537,
 * a2 = 1.5397677311665408, tajima_d = -1.4461719856148525.)
 *
 * v2m_diversity_of_counts (device form).  d_counts_a, and for the between form d_counts_b, are tables in device memory, 16-byte
 * aligned, plane_pitch % 4 == 0 and plane_pitch >= (L + 3) & ~3; they are read below element (L + 3) & ~3 of planes 0-3 only and left as
 * they were.  bounds is host memory, relative to the tables, bounds[n_bins] <= L.  d_bins (n_bins records) and d_sfs (u64[n_a / 2 + 1];
 * may be NULL, and must be in the between form) are device memory, 16-byte aligned; they are overwritten and nothing else is touched.
 * No graph is needed.  v2m_window_diversity (host form).  The tables are counted from rows_a and, for the between form, rows_b over
 * the view in force (the whole row or the column window; a window set is ignored), as v2m_column_counts counts them; bounds is
 * absolute and must lie inside the view; bins (n_bins records) and sfs (NULL, or u64[rows_a->n_rows / 2 + 1]) are host memory.  info,
 * which may be NULL, receives L, n_bins, multiallelic and -- while v2m_profile_enable is on, else 0 -- the stream time of the counts
 * and of the reduction, measured as for the pair distances (counts_ms is 0 in the device form).  Both are synchronous.
 * Errors, as for the other analyses: V2M_ERR_INVALID_ARGUMENT for NULL pointers, descending bounds, bounds outside the table or the
 * view, a misaligned pointer or a bad pitch, n_b != 0 without a second table, a spectrum in the between form; V2M_ERR_STATE without a
 * graph and V2M_ERR_PRECONDITION for bad cuts (host form).  n_bins == 0, or a group of 0 rows, returns V2M_OK and touches nothing (info
 * included).  The column window, the window set and what v2m_column_counts returns afterwards are left as they were.
 * The driver (--output-diversity, --diversity-sfs, --output-divergence) cuts the reference range into steps of --diversity-step
 * positions; the bin of a step begins at the column of its first position (columns_of_reference_range), so the columns of an insertion
 * fall to the bin of the reference position before them.  A window is --diversity-window / --diversity-step consecutive bins summed
 * field by field as integers; the doubles come after.
 * How (csrc/diversity_kernels.hpp).  diversity_init_kernel writes every record's `columns` and zeroes its sums; diversity_bins_kernel:
 * a lane takes four adjacent columns (one 16-byte load per plane), a workgroup a tile of 1 024; a tile inside one bin is a plain
 * workgroup reduction; otherwise the lanes find their bins by binary search of the bounds (a device copy) and sums that share a bin
 * meet in the wave by shuffles before one integer atomicAdd per wave, bin and field.  The spectrum goes through 4 096 u32 counters in
 * LDS when n / 2 + 1 fits, else straight to global atomics.  No V2M_KERNEL_* ids: V2M_KERNEL_LIMIT keeps its value. */
#define V2M_DIVERSITY_MAX_ROWS 32768u

typedef struct {
	uint64_t columns, called, diffs, pairs, segregating, complete, complete_segregating, complete_diffs;
} v2m_diversity_bin;             /* 64 bytes */

typedef struct { uint64_t columns, called, diffs, pairs; } v2m_diversity_between_bin;   /* 32 bytes */

typedef struct {
	uint64_t n_columns;      /* L */
	uint64_t n_bins;
	uint64_t multiallelic;   /* complete columns of three or four letters in [bounds[0], bounds[n_bins]); 0 without a spectrum */
	double counts_ms;        /* the column counts of the group or groups: stream time elapsed over the stage */
	double bins_ms;          /* diversity_init_kernel, diversity_bins_kernel and the zeroing of the spectrum: likewise */
} v2m_window_diversity_info;     /* 40 bytes */

int v2m_diversity_of_counts(v2m_ctx *ctx, const void *d_counts_a, const void *d_counts_b /* NULL: within */, uint64_t plane_pitch, uint64_t L,
                            uint64_t n_a, uint64_t n_b, const uint64_t *bounds /* host, relative */, uint64_t n_bins, void *d_bins,
                            void *d_sfs /* NULL, and NULL in the between form */, v2m_window_diversity_info *info /* may be NULL */);

int v2m_window_diversity(v2m_ctx *ctx, const v2m_row_batch *rows_a, const v2m_row_batch *rows_b /* NULL: within */,
                         const uint64_t *bounds /* host, absolute columns inside the view in force */, uint64_t n_bins, void *bins /* host */,
                         uint64_t *sfs /* host or NULL */, v2m_window_diversity_info *info /* may be NULL */);

/* ---- founder search: the chunk walks ---------------------------------- */

/* The edge-by-edge part of find_initial_cut_positions_lambda_min (libvcf2multialign/find_cut_positions.cc:126-176): the pBWT
 * steps of pbwt_context::update_divergence (include/vcf2multialign/pbwt.hh:77-134) and, at every candidate cut node, the walk
 * over the distinct divergence values from the largest down (find_cut_positions.cc:134-165) -- for chunks of consecutive
 * candidates whose start state the caller has built (the state after k edges is the copies sorted by their reversed k-edge
 * prefixes plus their divergence values; csrc/host/founder.cc builds it from the transposed matrix).  One workgroup walks
 * one chunk; the score updates of find_cut_positions.cc:55-63, which depend on each other, stay with the caller.
 *
 * The ctx must hold the uploaded graph WITH its path matrix (v2m_upload_graph with paths_by_chrom_copy_and_edge): the first
 * v2m_pbwt_* call after a matrix is bound transposes it back to edge-major bits on the device, and that copy (as large as the
 * matrix) is kept for the following v2m_pbwt_* calls -- one founder run makes two -- until the matrix is bound anew, a v2m_splice_rows*
 * call starts (the output that follows the searches gets the memory back) or the ctx is destroyed.  The copy is made from the matrix as it
 * is at that first call: a caller that changes a v2m_set_paths_device() matrix in place must bind it again before the next search.
 * n_copies <= 20480 and a bound matrix of at most 20480 copy columns (V2M_ERR_UNSUPPORTED beyond: a workgroup keeps the pBWT state
 * and one edge column in LDS; v2m_pbwt_cut_records as well: its class arrays sit beside them up to 12288 copies and in device memory above).  V2M_ERR_INVALID_ARGUMENT for candidate edges that decrease or lie outside the graph, aligned
 * positions that decrease (find_cut_positions.cc:129,151) and start_order entries >= n_copies -- checked on the host before any
 * kernel indexes with them.
 *   cand_edge[c], cand_aligned_pos[c]   of all n_candidates candidates: the index of the node's first ALT edge (ascending, one
 *                                       candidate per distinct edge index, :129) and the node's aligned position (:151)
 *   chunk_first[k] .. chunk_first[k+1]  the candidates of chunk k (n_chunks + 1 entries, ascending, chunk_first[0] >= 1)
 *   start_order, start_divergence       [n_chunks][n_copies]: the state after the first cand_edge[chunk_first[k]] edges;
 *                                       divergence values BIASED by one (0 = the reference's DIVERGENCE_MAX, pbwt.hh:25-42)
 * Outputs (host): for chunk k up to trial_capacity pairs at trial_pred / trial_class_count + k * trial_capacity -- (earlier
 * candidate, class count) in the order the reference's loop tries them --, trial_end[c] = the pairs of c's chunk up to and
 * including candidate c (written for the candidates of this call's chunks only), and chunk_status[k] = 0, or 1 when the chunk was left undone (more than 1024 distinct bins at one
 * node -- the candidates its divergence values other than the largest point to, the node itself and "none of them" counted --, or
 * trial_capacity exceeded): the caller walks that chunk itself; its trial_end entries and its pairs are unspecified.  Synchronous. */
int v2m_pbwt_cut_trials(v2m_ctx *ctx, uint64_t n_copies, uint64_t min_distance,
	uint64_t n_candidates, const uint32_t *cand_edge, const uint64_t *cand_aligned_pos,
	uint64_t n_chunks, const uint64_t *chunk_first, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t trial_capacity, uint32_t *trial_pred, uint32_t *trial_class_count, uint64_t *trial_end, uint32_t *chunk_status);

/* The same walks with the pairs handed over chunk by chunk instead of landing in arrays of the caller's: once all chunks are
 * walked, runs of whole chunks come back through two pinned slots of the library's in turn, and `sink` is called once per chunk,
 * in chunk order, on the calling thread -- (user, chunk index, status as above, the chunk's pairs, their number; the pointers are
 * valid during the call only; 0 pairs for a chunk left undone or empty) -- while the next slice is crossing the link.  trial_end
 * and chunk_status are complete before the first call.  The caller's score updates (find_cut_positions.cc:55-63) thus run under the
 * copies, and no large pageable array is ever a copy target (config 4: 800 MB of pairs; touching, pinning and releasing such an
 * array cost more than using it).  A sink that returns non-zero ends the call with V2M_ERR_SINK. */
typedef int (*v2m_trials_sink)(void *user, uint64_t chunk, uint32_t status, const uint32_t *pred, const uint32_t *class_count, uint64_t n_pairs);
int v2m_pbwt_cut_trials_streamed(v2m_ctx *ctx, uint64_t n_copies, uint64_t min_distance,
	uint64_t n_candidates, const uint32_t *cand_edge, const uint64_t *cand_aligned_pos,
	uint64_t n_chunks, const uint64_t *chunk_first, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t trial_capacity, uint64_t *trial_end, uint32_t *chunk_status, v2m_trials_sink sink, void *sink_user);

/* The same for founder_sequence_greedy_output::find_matchings (libvcf2multialign/founder_sequence_greedy_output.cc:154-512): the
 * pBWT steps between cut positions and, at every cut, what the reference's loop :215-251 collects -- the number of path classes
 * of the block that ends there, the first copy in pBWT order and whether it followed REF edges only (:454-462), and the joined
 * classes {class in the previous block, class in this block, copies} of the two-block span, in pBWT order (the caller sorts
 * them by size, :256, and runs the greedy assignment, :254-457, which is strictly sequential).
 *   cut_edge[j]                   ALT edges before cut node j (alt_edge_count_csum[cut_positions[j]]), ascending, n_cuts entries
 *   chunk_first_cut[k] .. [k+1]   the cuts chunk k handles (>= 1); start_edge[k] <= cut_edge[chunk_first_cut[k] - 1]: the given
 *                                 state (start_order / start_divergence, [n_chunks][n_copies], divergence biased) is the one after
 *                                 that many edges; the kernel walks on to the cut before the chunk's first one by itself
 * Outputs (host): per chunk up to pool_capacity joined classes at pool_lhs / pool_rhs / pool_size + k * pool_capacity
 * (0xFFFFFFFF = PLOIDY_MAX, "no class"); per cut j >= 1 rec_pool_end[j] (the chunk's joined classes up to and including cut j),
 * rec_distinct[j], rec_first_class[j], rec_first_is_ref[j]; chunk_status[k] = 0, or 1 when the chunk was left undone
 * (pool_capacity exceeded).  Same requirements on the ctx and the start states as v2m_pbwt_cut_trials; cut edges that decrease or
 * lie outside the graph are V2M_ERR_INVALID_ARGUMENT, and so is cut_edge[j] == cut_edge[j - 2]: no copy starts a class of a two-block
 * span without an edge (the reference asserts there, :245).  Two cuts in a row with the same edge count are taken: no copy that
 * has matched another one starts a class of the block between them (0xFFFFFFFF on that side of its joined classes); csrc/host
 * refuses such cut lists before it gets here, as the reference's assertions do.  Synchronous. */
int v2m_pbwt_cut_records(v2m_ctx *ctx, uint64_t n_copies, uint64_t n_cuts, const uint32_t *cut_edge,
	uint64_t n_chunks, const uint64_t *chunk_first_cut, const uint32_t *start_edge, const uint32_t *start_order, const uint32_t *start_divergence,
	uint64_t pool_capacity, uint32_t *pool_lhs, uint32_t *pool_rhs, uint32_t *pool_size,
	uint64_t *rec_pool_end, uint32_t *rec_distinct, uint32_t *rec_first_class, uint32_t *rec_first_is_ref, uint32_t *chunk_status);

/* ---- BGZF output --------------------------------------------------------------------------------
 *
 * BGZF is the blocked gzip of the SAM/BAM specification, section 4.1; any gzip reader reads it, htslib indexes it.
 *   - Output = a sequence of members.  Each member is a gzip member (RFC 1952) with FLG.FEXTRA set and one extra subfield 'B' 'C'
 *     of SLEN 2 holding BSIZE = the member's total length - 1; a member is at most 65 536 bytes and holds at most 65 280
 *     uncompressed bytes (0xff00).  The footer holds the CRC-32 (IEEE, reflected 0xEDB88320) and ISIZE.
 *   - The deflate payload is one final block: dynamic Huffman (BTYPE 10) over zlib's Z_RLE tokens (literals and distance-1
 *     matches), or stored (BTYPE 00) when that is not larger.  Compressed bytes need not match zlib's; decompressed ones do.
 *   - A file ends with the 28-byte EOF member 1f 8b 08 04 00 00 00 00 00 ff 06 00 42 43 02 00 1b 00 03 00 00 00 00 00 00 00 00 00.
 *   - Row bodies: every row's body is cut into 65 280-byte pieces from its first byte, one member each (an empty body gives no
 *     member).  So the decompressed bytes of a row's members are exactly its body, and an A2M file written with V2M_SPLICE_BGZF
 *     is its plain bytes: the glue around the bodies ('>'id'\n' before, '\n' after) in stored members of
 *     v2m_bgzf_frame_stored, then the EOF member. */

/* Bytes that frame_stored or compress can write for n input bytes at most (n + 31 per 65 280-byte piece; 28 for n = 0). */
uint64_t v2m_bgzf_bound(uint64_t n);

/* Frames n host bytes as stored-block BGZF members (host only, no ctx or device); n = 0 writes exactly the EOF member.
 * V2M_ERR_INVALID_ARGUMENT when cap is smaller than what the framing needs. */
int v2m_bgzf_frame_stored(const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out);

/* Compresses n host bytes to BGZF members on the GPU, through the kernels V2M_SPLICE_BGZF uses.  Synchronous; n = 0 writes nothing
 * (no EOF member).  V2M_ERR_INVALID_ARGUMENT when the members do not fit into cap (v2m_bgzf_bound(n) always does). */
int v2m_bgzf_compress(v2m_ctx *ctx, const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out);

/* ---- BGZF input ---------------------------------------------------------------------------------
 *
 * What v2m_bgzf_scan and v2m_bgzf_decompress accept (htslib's reader, and exactly zlib's inflate for the payload):
 *   - Members back to back.  A member has the header bgzip writes: 1f 8b 08 04 (CM 8, FLG exactly FEXTRA), any MTIME, XFL and OS,
 *     XLEN = 6 and one subfield 'B' 'C' of SLEN 2 holding BSIZE = the member's length - 1.  The deflate payload is bytes
 *     [18, BSIZE + 1 - 8) of the member; the footer is CRC-32 (IEEE, reflected 0xEDB88320), then ISIZE <= 65 536.
 *   - The payload is any RFC 1951 stream that zlib's inflate accepts: stored, fixed and dynamic Huffman blocks, any number of them,
 *     distances up to 32 768 within the member (a member is inflated on its own; no window crosses members).  Refused as zlib refuses
 *     them: block type 3; LEN != ~NLEN; HLIT > 286 or HDIST > 30; an over-subscribed code, or an incomplete one (a literal/length or
 *     distance code may be incomplete only as a single code of length 1; the code-length code never); no end-of-block code; a repeat
 *     code 16 with no previous length, or a repeat past HLIT + HDIST; length symbols 286 / 287 and distance symbols 30 / 31; a distance
 *     before the member's first byte.  Also refused: output longer than ISIZE, a stream that reads past the payload, output shorter
 *     than ISIZE, a CRC-32 that does not match.  Bytes after the final block inside the payload are ignored, as zlib leaves them.
 *   - The members decompress to the concatenation of their bytes; the 28-byte EOF member and other empty members add nothing.
 *   - Gzip that is not BGZF (the first member's header is gzip's, without the BC subfield) is V2M_ERR_UNSUPPORTED: the message says
 *     so and that the file has to be recompressed with bgzip.  Broken framing and corrupt members are V2M_ERR_INVALID_ARGUMENT; the
 *     message gives the compressed offset of the first bad member and what is wrong with it.
 * n = 0 is an empty input: no members, no bytes. */

/* Host only, no ctx: walks the BSIZE chain and checks the framing above (not the payloads); members, total decompressed bytes,
 * whether the last member is the EOF member.  Messages go to v2m_last_error(NULL) on the calling thread. */
int v2m_bgzf_scan(const void *src, uint64_t n, uint64_t *n_members_out, uint64_t *n_bytes_out, int *ends_with_eof_out);

/* Inflates n host bytes of BGZF into dst (cap bytes of ordinary host memory) on the GPU; *n_out = the decompressed bytes.  Synchronous.
 * A cap below what v2m_bgzf_scan reports is V2M_ERR_INVALID_ARGUMENT.  The framing is checked on the host first, every payload, CRC-32
 * and ISIZE on the GPU (bgzf_inflate_kernel: one wave per member, the member's output in LDS).  Works in slices of whole members
 * through the context's two streams and pinned slots (V2M_RING_SLOT_BYTES caps a slice, as for the row calls): the H2D copy of the
 * next slice and the D2H copy of the previous one run under the kernel of the current one.  On failure dst holds an unspecified
 * prefix. */
int v2m_bgzf_decompress(v2m_ctx *ctx, const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out);

/* ---- VCF scan ------------------------------------------------------------------------------------
 *
 * v2m_vcf_scan turns VCF text (plain, or BGZF inflated on the device) into what a graph builder needs of it without the text ever
 * reaching the host: per line a record, for some lines a head (bytes of the line), and for the records on the wanted chromosome
 * bit columns in the layout of paths_by_edge_and_chrom_copy (row r = bit r & 63 of word r >> 6 of a column).
 *
 * Lines.  A line is the bytes between '\n's; a last line without '\n' counts, a trailing '\n' adds no empty line.
 *
 * Kinds.  n_samples and ploidy(s) = copy_begin[s + 1] - copy_begin[s] come from the layout (below).
 *   0  the line is empty or its first byte is '#'.  No head, except for a line that starts with "#CHROM": its whole text.
 *   3  (declined) fewer than 7 tabs.  Head = the whole line.
 *   1  column 1 is not wanted_chr.  No head.
 *   2  (parsed) all of a - e hold.  Head = the bytes before the 9th tab (CHROM ... FORMAT); n_alts columns from column_begin on,
 *      column a - 1 with bit `row` set exactly when an included copy `row` carries allele a >= 1.
 *        a. the last byte is not '\r';
 *        b. at least 9 tabs, and column 9 is "GT" or begins with "GT:";
 *        c. column 5 has 1 to 8 comma-separated entries: n_alts = its commas + 1 (what the entries are is the caller's business);
 *        d. exactly 8 + n_samples tabs;
 *        e. for every sample s and every token index c < ploidy(s) the token exists and is "." or 1 - 3 decimal digits with value
 *           <= n_alts.  Tokens: the sample column up to its first ':', split at '|' and '/'.  Tokens at c >= ploidy(s) are not
 *           looked at.
 *   3  otherwise.  Head = the whole line, no columns.  Declining is always safe: the caller parses the line from its text.
 * Every record has head_offset = the head bytes and column_begin = the columns of the chunk's lines before it; n_alts is 0 unless
 * the kind is 2.  The chunk's heads are exactly its lines' heads in line order, its n_columns the sum of its lines' n_alts -- also
 * when words_per_column is 0 (a layout that includes no copy): the columns then have no words, and they are counted all the same.
 *
 * Layout.  The first line that is not of kind 0 and whose column 1 (up to the first tab; without a tab the whole line less a final
 * '\r') is wanted_chr fixes the layout: `layout` is called exactly once, with that line's whole text, before any genotype of its
 * slice is looked at.  The arrays it returns must stay valid until v2m_vcf_scan returns.  copy_begin must not decrease, row_lookup
 * entries are -1 (copy not included) or < n_rows, n_rows <= 64 * words_per_column.  Lines before the layout line are of kinds 0, 1 or
 * 3 by construction; when no line is a layout line, `layout` is never called.
 * n_rows above 32 768 (or words_per_column above 512) is V2M_ERR_UNSUPPORTED.
 *
 * Chunks.  `chunk` is called once per slice, in file order, with whole lines only; a line that straddles a slice seam is carried
 * to the next slice on the device.  One slice is the exception: the slice that holds the layout line is delivered as two chunks, the
 * lines before the layout line (none: no such chunk) and, after `layout` has run, the lines from it on, so that the caller has seen
 * every earlier line (the #CHROM line with the sample names among them) when `layout` is called.  A chunk therefore lies wholly
 * before the layout line (words_per_column = 0, no columns) or wholly from it on.  A slice without a whole line gives no chunk.
 * A slice's text (the carried bytes included) is at most V2M_RING_SLOT_BYTES (default 64 MiB; for
 * BGZF, whole members: 64 KiB more when one member needs it); a line that does not fit into a slice's text makes the call return
 * V2M_ERR_UNSUPPORTED.  Everything a chunk points to is pinned memory of the library's, valid only during the callback.
 *
 * src is BGZF when it starts with 1f 8b: then the framing and payload rules, codes and messages are those of v2m_bgzf_scan /
 * v2m_bgzf_decompress.  Otherwise it is plain text.  A non-zero return from either callback ends the scan with V2M_ERR_SINK.
 * Synchronous.  Nothing else of the context changes: a resident graph, a column window and output buffers are untouched. */

typedef struct v2m_vcf_line {
	uint32_t kind;         /* 0 - 3 */
	uint32_t n_alts;       /* kind 2: 1 - 8; else 0 */
	uint32_t head_offset;  /* into v2m_vcf_chunk.heads */
	uint32_t head_length;
	uint64_t column_begin; /* first of the line's n_alts columns */
} v2m_vcf_line;

typedef struct v2m_vcf_layout {
	uint32_t n_samples;
	uint32_t n_rows;              /* included chromosome copies */
	uint64_t words_per_column;    /* of paths_by_edge_and_chrom_copy (its rows are padded) */
	const uint32_t *copy_begin;   /* [n_samples + 1]: the copies of sample s are row_lookup[copy_begin[s] .. copy_begin[s + 1]) */
	const int32_t *row_lookup;    /* [copy_begin[n_samples]]: the row of a copy, or -1 when it is not included */
} v2m_vcf_layout;

typedef struct v2m_vcf_chunk {
	uint64_t first_line;          /* file-wide 0-based index of the chunk's first line */
	uint64_t n_lines;
	const v2m_vcf_line *lines;    /* [n_lines] */
	const char *heads;
	uint64_t head_bytes;
	const uint64_t *columns;      /* [n_columns][words_per_column] */
	uint64_t n_columns;
	uint64_t words_per_column;    /* 0 before the layout is known */
} v2m_vcf_chunk;

typedef int (*v2m_vcf_layout_fn)(void *user, uint64_t line_index, const char *line, uint64_t length, v2m_vcf_layout *out);
typedef int (*v2m_vcf_chunk_fn)(void *user, const v2m_vcf_chunk *chunk);

int v2m_vcf_scan(v2m_ctx *ctx, const void *src, uint64_t n, const char *wanted_chr, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user);

/* ---- verification helper ------------------------------------------------------------------ */

/* 64-bit position-sensitive checksum of each of n_rows device rows (row i = d_rows + i*row_pitch,
 * lengths[i] bytes, or `length` for all rows when lengths == NULL; d_rows and row_pitch multiples of 8):
 *   the row is read as 8-byte little-endian words w[0 .. ceil(len/8)), the last one zero-padded past the row's end;
 *   checksum = sum over k of mix64((k + 1) * 0x9E3779B97F4A7C15 ^ w[k])  +  mix64(len)   (mod 2^64),
 *   mix64 = the splitmix64 finaliser (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31).
 * Used to check full-size outputs against the CPU without moving them.  Synchronous. */
int v2m_checksum_rows_device(v2m_ctx *ctx, const void *d_rows, uint64_t row_pitch, uint64_t n_rows, uint64_t length, const uint64_t *lengths, uint64_t *checksums_out);

/* ---- kernel timing ------------------------------------------------------------------------ */

enum {
	V2M_KERNEL_TRANSPOSE = 0,       /* transpose_bits_kernel */
	V2M_KERNEL_RESOLVE = 1,         /* resolve_effective_edges_kernel (per-row skip-rule scan) */
	V2M_KERNEL_SPLICE_ALIGNED = 2,  /* splice_aligned_kernel (dominant) */
	V2M_KERNEL_SPLICE_UNALIGNED = 3, /* splice_unaligned_kernel (pass 2 of unaligned mode: build + compact the tiles) */
	V2M_KERNEL_TEMPLATE = 4,        /* expand_reference_row_kernel (once per upload) */
	V2M_KERNEL_UNALIGNED_COUNT = 5, /* count_unaligned_kernel + scan_tile_counts_kernel (pass 1 of unaligned mode) */
	V2M_KERNEL_BGZF = 6,            /* bgzf_deflate_kernel + bgzf_scan_kernel + bgzf_compact_kernel (V2M_SPLICE_BGZF, v2m_bgzf_compress) */
	V2M_KERNEL_INFLATE = 7,         /* bgzf_inflate_kernel (v2m_bgzf_decompress), one launch per slice */
	V2M_KERNEL_VCF = 8,             /* the line index, head and genotype launches of one slice of v2m_vcf_scan, as one group */
	V2M_KERNEL_COUNT = 9
};
/* The passes of v2m_row_ops, added behind the ids above (V2M_KERNEL_COUNT keeps counting those; V2M_KERNEL_END bounds what
 * v2m_profile_get accepts).  The call's count_unaligned_kernel + scan_tile_counts_kernel launches are timed as V2M_KERNEL_UNALIGNED_COUNT. */
enum {
	V2M_KERNEL_ROW_OPS_COUNT = 9,   /* count_row_ops_kernel (pass 1: breakpoints, first and last class per row tile) */
	V2M_KERNEL_ROW_OPS_SCAN = 10,   /* scan_row_ops_kernel (pass 2: op offsets and carried classes per row) */
	V2M_KERNEL_ROW_OPS_EMIT = 11,   /* emit_row_ops_kernel (pass 3: the breakpoint records) */
	/* v2m_splice_window_set_distinct, per slice: one group of hash launches, then per round one of gather and one of verify launches */
	V2M_KERNEL_DISTINCT_HASH = 12,  /* hash_pieces_kernel */
	V2M_KERNEL_DISTINCT_GATHER = 13, /* gather_pieces_kernel */
	V2M_KERNEL_DISTINCT_VERIFY = 14, /* verify_pieces_kernel */
	V2M_KERNEL_END = 15
};
/* The passes of v2m_column_counts[_device], added behind those in the same way (V2M_KERNEL_END keeps its value; V2M_KERNEL_LIMIT
 * bounds what v2m_profile_get accepts). */
enum {
	V2M_KERNEL_COLUMN_COUNTS = 15,  /* column_counts_kernel, one launch per slice */
	V2M_KERNEL_COLUMN_SELECT = 16,  /* count_variable_columns_kernel + scan_tile_counts_kernel + emit_column_counts_kernel, one group per column range */
	V2M_KERNEL_LIMIT = 17
};

/* When enabled, every launch of the kernels above is bracketed by HIP events on the ctx's
 * stream.  v2m_profile_get() synchronises and returns launch count and summed device time. */
int v2m_profile_enable(v2m_ctx *ctx, int enabled);
int v2m_profile_reset(v2m_ctx *ctx);
int v2m_profile_get(v2m_ctx *ctx, int kernel, uint64_t *launches_out, double *total_ms_out);
/* Per-launch device times (ms) in launch order; writes min(capacity, launches) values, returns the launch count in *launches_out. */
int v2m_profile_get_launches(v2m_ctx *ctx, int kernel, double *ms_out, uint64_t capacity, uint64_t *launches_out);

#ifdef __cplusplus
}
#endif

#endif /* V2M_HIP_H */
