#include "readers.hh"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <chrono>
#include <algorithm>
#include <memory>
#include <exception>
#include <functional>
#include <cstring>
#include <fstream>
#include <mutex>
#include <stdexcept>
#include <thread>

#include "graph_builder.hh"

namespace v2m::host {

bool read_single_fasta_sequence(char const *path, sequence_type &seq, char const *seq_id)
{
	std::ifstream is(path, std::ios::binary);
	if (!is) return false;
	seq.clear();
	std::string line;
	bool wanted(false), found(false);
	while (std::getline(is, line)) {
		if (!line.empty() && '\r' == line.back()) line.pop_back();
		if (!line.empty() && '>' == line.front()) {
			if (found) break;
			auto const stop(line.find_first_of(" \t", 1));
			std::string_view const id(std::string_view(line).substr(1, std::string::npos == stop ? std::string::npos : stop - 1));
			wanted = !seq_id || id == seq_id;
			found = wanted;
			continue;
		}
		if (wanted) seq.insert(seq.end(), line.begin(), line.end());
	}
	return found;
}

// Lines as std::getline splits them: at '\n', the last one without it, no empty line after a final '\n'.
bool read_single_fasta_sequence(std::string_view text, sequence_type &seq, char const *seq_id)
{
	seq.clear();
	bool wanted(false), found(false);
	std::size_t pos(0);
	while (pos < text.size()) {
		std::size_t eol(text.find('\n', pos));
		if (std::string_view::npos == eol) eol = text.size();
		std::string_view line(text.substr(pos, eol - pos));
		pos = eol + 1;
		if (!line.empty() && '\r' == line.back()) line.remove_suffix(1);
		if (!line.empty() && '>' == line.front()) {
			if (found) break;
			auto const stop(line.find_first_of(" \t", 1));
			std::string_view const id(line.substr(1, std::string_view::npos == stop ? std::string_view::npos : stop - 1));
			wanted = !seq_id || id == seq_id;
			found = wanted;
			continue;
		}
		if (wanted) seq.insert(seq.end(), line.begin(), line.end());
	}
	return found;
}


mapped_file::mapped_file(char const *path)
{
	fd = ::open(path, O_RDONLY);
	if (fd < 0) throw std::runtime_error(std::string("unable to open ") + path);
	struct stat st;
	if (0 != ::fstat(fd, &st)) { ::close(fd); throw std::runtime_error(std::string("unable to stat ") + path); }
	size = std::size_t(st.st_size);
	if (size) {
		void *p(::mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0));
		if (MAP_FAILED == p) { ::close(fd); throw std::runtime_error(std::string("unable to map ") + path); }
		data = static_cast<char const *>(p);
		::madvise(p, size, MADV_SEQUENTIAL);
	}
}

mapped_file::~mapped_file()
{
	if (data) ::munmap(const_cast<char *>(data), size);
	if (fd >= 0) ::close(fd);
}


namespace {

// Splits [begin, end) at `delim` without allocating: call next() until it returns false.
struct field_cursor {
	char const *p, *end;
	char delim;
	bool done{false};
	field_cursor(std::string_view s, char d) : p(s.data()), end(s.data() + s.size()), delim(d) {}
	bool next(std::string_view &out)
	{
		if (done) return false;
		char const *q(static_cast<char const *>(std::memchr(p, delim, std::size_t(end - p))));
		if (!q) { out = std::string_view(p, std::size_t(end - p)); done = true; return true; }
		out = std::string_view(p, std::size_t(q - p));
		p = q + 1;
		return true;
	}
};

[[noreturn]] void bad(u64 lineno, char const *what)
{
	throw std::runtime_error("VCF line " + std::to_string(lineno) + ": " + what);
}

// ---- record parsing (runs on worker threads) ------------------------------------------------------------------

// What a worker leaves behind for a chunk.  Besides the records themselves, everything their genotypes amount to (at population
// scale the genotypes ARE the work: config 3 has 360 M of them), so that the one thread that merges chunks in file order never
// looks at a genotype:
//   - the path bits, as the chunk's own slice of paths_by_edge_and_chrom_copy: one column per ALT that becomes an edge (the
//     builder numbers the edges of consecutive records, and of a record's ALTs, consecutively: variant_graph.cc:328-364), in the
//     matrix's own layout, so merging them is one memcpy;
//   - per chromosome copy, its first ALT in the chunk (record, allele) and the reference position its last one reaches
//     (variant_graph.cc:422-423): what the overlap check (:408-418) of the NEXT chunk's first ALT of that copy needs, and what
//     this chunk's needs from the previous ones;
//   - the overlaps that lie inside the chunk (a copy's second, third, ... ALT here), in the reference's order.
struct chunk_overlap { u32 record, row, alt_number; };               // record = index in the chunk

struct parsed_record {
	u64 line_in_chunk;        // 1-based within the chunk
	u64 data_line_in_chunk;   // counts only non-header lines
	u64 ref_pos;
	std::string_view id, ref;
	u32 alt_begin, n_alts;
	u64 first_column;         // columns of the chunk's bit slice before this record's
	u64 overlap_begin;        // overlaps inside the chunk before this record's
	u64 chr_mismatches_before;   // records of other chromosomes seen in the chunk before this one
};

constexpr u32 kNoRecord = UINT32_MAX;

struct parsed_chunk {
	std::vector<parsed_record> records;
	std::vector<alt_allele> alts;
	std::vector<u64> bits;                      // [columns][words per column]
	u64 n_columns{};
	std::vector<u32> first_record, first_alt;   // per chromosome copy (row); kNoRecord: no ALT in this chunk
	std::vector<u64> last_target;               // per row, valid where first_record is
	std::vector<chunk_overlap> overlaps;
	u64 n_lines{}, n_data_lines{}, chr_mismatches{};
	std::string error;        // first error, with its chunk-relative line in error_line
	u64 error_line{};
};

struct parse_context {
	std::string_view wanted_chr;
	std::size_t n_samples{};
	// (sample, copy) -> row of paths_by_edge_and_chrom_copy, or -1 when the copy is not included;
	// copies of sample s are row_lookup[copy_begin[s] .. copy_begin[s + 1])
	std::vector<std::int32_t> row_lookup;
	std::vector<u32> copy_begin;
	u64 n_rows{};               // included chromosome copies
	u64 words_per_column{};     // of paths_by_edge_and_chrom_copy (its rows are padded)
};

struct chunk_error { u64 line; char const *what; };

// "0|0\t" and "0/0\t" as the four bytes a little-endian load sees
constexpr std::uint32_t kRefRefPhased = 0x09307C30u, kRefRefUnphased = 0x09302F30u;
static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the column fast path compares little-endian words");

// The parser of one chunk, a line at a time: the head part (the first nine columns: POS, ID, REF, the ALTs and their columns, FORMAT) and
// the genotype application part (bits, first_record, first_alt, last_target, overlaps), which the text path feeds from the sample columns
// and the scanned path (readers.hh) from bit columns.
struct chunk_parser {
	parse_context const &ctx;
	parsed_chunk &out;
	std::vector<u64> alt_column;                 // of the record at hand: ALT -> column of the chunk's slice, or UINT64_MAX (no edge)
	u64 columns_before_record{};
	std::size_t overlaps_before_record{};
	// the record at hand
	parsed_record rec{};
	std::size_t gt_index{};
	u32 rec_index{};
	u64 target_ref_pos{};

	chunk_parser(parse_context const &c, parsed_chunk &o) : ctx(c), out(o)
	{
		out.bits.clear();
		out.n_columns = 0;
		out.overlaps.clear();
		out.first_record.assign(ctx.n_rows, kNoRecord);
		out.first_alt.assign(ctx.n_rows, 0);
		out.last_target.assign(ctx.n_rows, 0);
	}

	// The head part, after the line has been counted: false for a record of another chromosome (counted, nothing else to do).
	bool head(field_cursor &fc)
	{
		std::string_view chrom, pos_f, id, ref, alt_f, skip, format;
		if (!(fc.next(chrom) && fc.next(pos_f) && fc.next(id) && fc.next(ref) && fc.next(alt_f) && fc.next(skip) && fc.next(skip) && fc.next(skip)))
			throw chunk_error{out.n_lines, "fewer than 8 columns"};
		if (chrom != ctx.wanted_chr) { ++out.chr_mismatches; return false; }          // variant_graph.cc:203-207
		if (!fc.next(format)) throw chunk_error{out.n_lines, "variant does not have a genotype"};   // :209-213
		gt_index = SIZE_MAX;
		{
			field_cursor ff(format, ':');
			std::string_view f;
			for (std::size_t i(0); ff.next(f); ++i) if (f == "GT") { gt_index = i; break; }
			if (SIZE_MAX == gt_index) throw chunk_error{out.n_lines, "variant does not have a genotype"};
		}

		rec = parsed_record{};
		rec.line_in_chunk = out.n_lines;
		rec.data_line_in_chunk = out.n_data_lines;
		rec.chr_mismatches_before = out.chr_mismatches;
		rec.id = id;
		rec.ref = ref;
		if (pos_f.empty()) throw chunk_error{out.n_lines, "empty POS"};
		for (char const c : pos_f) { if (c < '0' || '9' < c) throw chunk_error{out.n_lines, "bad POS"}; rec.ref_pos = 10 * rec.ref_pos + u64(c - '0'); }
		if (0 == rec.ref_pos) throw chunk_error{out.n_lines, "POS must be 1-based"};
		--rec.ref_pos;                                                                 // zero_based_pos (:292)

		rec.alt_begin = u32(out.alts.size());
		{
			field_cursor ac(alt_f, ',');
			for (std::string_view a; ac.next(a);) out.alts.push_back({classify_alt(a), a});
		}
		rec.n_alts = u32(out.alts.size()) - rec.alt_begin;
		// the ALTs that become edges get the chunk's next columns, in ALT order (variant_graph.cc:328-364)
		rec.first_column = columns_before_record = out.n_columns;
		rec.overlap_begin = overlaps_before_record = out.overlaps.size();
		alt_column.assign(rec.n_alts, UINT64_MAX);
		for (u32 a(0); a < rec.n_alts; ++a) if (alt_kind::unhandled != out.alts[rec.alt_begin + a].kind) alt_column[a] = out.n_columns++;
		out.bits.resize(out.n_columns * ctx.words_per_column, 0);
		rec_index = u32(out.records.size());
		target_ref_pos = rec.ref_pos + rec.ref.size();                                 // :333
		return true;
	}

	// The genotype application part: copy `row` carries ALT `allele` (1 <= allele <= rec.n_alts) of the record at hand.  Calls come in
	// ascending row order.
	void apply(u32 row, u32 allele)
	{
		u64 const column(alt_column[allele - 1]);
		if (UINT64_MAX != column) {                                   // (an ALT without an edge: :401-403)
			out.bits[column * ctx.words_per_column + (row >> 6)] |= u64(1) << (row & 63);   // :424
			note(row, allele);
		}
	}

	// The same without the bit (the scanned path copies whole columns).
	void note(u32 row, u32 allele)
	{
		if (kNoRecord == out.first_record[row]) { out.first_record[row] = rec_index; out.first_alt[row] = allele; }
		else if (rec.ref_pos < out.last_target[row]) out.overlaps.push_back({rec_index, row, allele});   // :408-418
		out.last_target[row] = target_ref_pos;                    // :422-423
	}

	// One line of text (without its '\n').
	void line(std::string_view line)
	{
		++out.n_lines;
		if (!line.empty() && '\r' == line.back()) line.remove_suffix(1);
		if (line.empty() || '#' == line.front()) return;
		++out.n_data_lines;

		field_cursor fc(line, '\t');
		if (!head(fc)) return;

		// genotypes of the included copies (:379-425); allele 0 and '.' change nothing (:393-397)
		std::size_t sample(0);
		for (std::string_view field; ; ++sample) {
			// Most of a population-scale VCF is "0|0\t": both copies on the reference allele, nothing to record (:393-397).  Runs of
			// such columns are skipped four bytes at a time instead of a memchr and three loops each (config 3: 2.5 G columns; GT must
			// be the first FORMAT key and the sample at most diploid, so that the general path below would find nothing either).
			if (0 == gt_index) {
				while (!fc.done && fc.end - fc.p >= 4 && sample < ctx.n_samples && ctx.copy_begin[sample + 1] - ctx.copy_begin[sample] <= 2) {
					std::uint32_t four;
					std::memcpy(&four, fc.p, 4);
					if (kRefRefPhased != four && kRefRefUnphased != four) break;
					fc.p += 4;
					++sample;
				}
			}
			if (!fc.next(field)) break;
			if (sample >= ctx.n_samples) throw chunk_error{out.n_lines, "more sample columns than in the header"};
			std::string_view gt(field);
			if (gt_index || std::string_view::npos != field.find(':')) {
				field_cursor sf(field, ':');
				std::size_t i(0);
				bool found(false);
				for (std::string_view f; sf.next(f); ++i) if (i == gt_index) { gt = f; found = true; break; }
				if (!found) throw chunk_error{out.n_lines, "sample without GT"};
			}
			u32 const c_begin(ctx.copy_begin[sample]), c_end(ctx.copy_begin[sample + 1]);
			u32 copy(0);
			std::size_t a(0);
			while (a <= gt.size()) {
				std::size_t b(a);
				while (b < gt.size() && '|' != gt[b] && '/' != gt[b]) ++b;
				if (c_begin + copy < c_end) {
					std::int32_t const row(ctx.row_lookup[c_begin + copy]);
					if (row >= 0) {
						std::string_view const tok(gt.substr(a, b - a));
						if (tok.empty()) throw chunk_error{out.n_lines, "empty GT allele"};
						if (tok != ".") {
							u32 allele(0);
							for (char const c : tok) { if (c < '0' || '9' < c) throw chunk_error{out.n_lines, "bad GT allele"}; allele = 10 * allele + u32(c - '0'); }
							if (allele) {
								if (allele > rec.n_alts) throw chunk_error{out.n_lines, "GT allele exceeds the ALT count"};
								apply(u32(row), allele);
							}
						}
					}
				}
				++copy;
				a = b + 1;
			}
			for (u32 c(copy); c_begin + c < c_end; ++c)                               // libbio_assert_lt(chr_idx_input, gt.size()), :390
				if (ctx.row_lookup[c_begin + c] >= 0) throw chunk_error{out.n_lines, "GT has fewer alleles than in the first record"};
		}
		if (sample != ctx.n_samples) throw chunk_error{out.n_lines, "sample column count differs from the header"};
		out.records.push_back(rec);
	}

	// A line of the scanned path whose genotypes are bit columns (v2m_hip.h: kind 2): `head_text` = its first nine columns, column a of
	// `columns` (words_per_column words each) = the rows that carry ALT a + 1.  The head goes through the same code as a line of text; the
	// columns of the ALTs that become edges are copied, and the rows are visited in ascending order across all of them, which is the order
	// in which the text parser meets them.
	void scanned_line(std::string_view head_text, u64 const *columns, u32 n_alts)
	{
		++out.n_lines;
		++out.n_data_lines;
		field_cursor fc(head_text, '\t');
		if (!head(fc)) return;                                                         // (never: the scan compared CHROM)
		if (n_alts != rec.n_alts) throw std::logic_error("VCF reader: the scan counted other ALTs than the parser");
		u64 const wpc(ctx.words_per_column);
		for (u32 a(0); a < n_alts; ++a)
			if (UINT64_MAX != alt_column[a] && wpc) std::memcpy(out.bits.data() + alt_column[a] * wpc, columns + a * wpc, wpc * sizeof(u64));
		for (u64 w(0); w < wpc; ++w) {
			u64 any(0);
			for (u32 a(0); a < n_alts; ++a) if (UINT64_MAX != alt_column[a]) any |= columns[a * wpc + w];
			for (; any; any &= any - 1) {
				u32 const bit(u32(__builtin_ctzll(any)));
				u32 allele(0);
				for (u32 a(0); a < n_alts && !allele; ++a) if (UINT64_MAX != alt_column[a] && ((columns[a * wpc + w] >> bit) & 1)) allele = a + 1;
				u64 const row(64 * w + bit);
				if (row >= ctx.n_rows) throw std::logic_error("VCF reader: the scan set a bit outside the rows");
				note(u32(row), allele);
			}
		}
		out.records.push_back(rec);
	}

	// What the failing record had claimed before it failed (the records before it are still merged; the per-copy state it may have
	// touched no longer matters: the error ends the build right after them).
	void failed(chunk_error const &e)
	{
		out.error = e.what;
		out.error_line = e.line;
		out.n_columns = columns_before_record;
		out.overlaps.resize(overlaps_before_record);
	}
};

// Parses the lines of text[begin, end) (whole lines) into `out`.
void parse_chunk(std::string_view text, parse_context const &ctx, parsed_chunk &out)
{
	chunk_parser parser(ctx, out);
	std::size_t pos(0);
	try {
		while (pos < text.size()) {
			std::size_t eol(text.find('\n', pos));
			if (std::string_view::npos == eol) eol = text.size();
			std::string_view const line(text.substr(pos, eol - pos));
			pos = eol + 1;
			parser.line(line);
		}
	} catch (chunk_error const &e) {
		parser.failed(e);
	}
}

// What the text path and the scanned path share around the chunks: the sample names of the #CHROM line, the first record on the requested
// chromosome (it fixes ploidy and inclusion, variant_graph.cc:215-288) and the merge stage.
struct graph_assembly {
	sequence_type const &ref_seq;
	std::string_view ref_sv;
	variant_graph &graph;
	build_graph_statistics &stats;
	build_graph_delegate &delegate;
	graph_builder builder;
	parse_context ctx;
	std::vector<std::string> vcf_sample_names;
	u64 lineno_base{}, var_idx{};
	std::vector<std::pair<u32, u32>> row_origin;                      // row of the path matrix -> (sample column, copy of it), for the overlap reports
	std::vector<u64> reaches;                                         // per copy: target_ref_positions_by_chrom_copy (:422-423)
	std::vector<chunk_overlap> reported;
	double t_records{}, t_genotypes{};

	graph_assembly(sequence_type const &ref, char const *chr_id, variant_graph &g, build_graph_statistics &st, build_graph_delegate &d, u64 path_alignment)
		: ref_seq(ref), ref_sv(ref.data(), ref.size()), graph((g = variant_graph{}, g)), stats(st), delegate(d), builder(g, /* track_paths */ true, path_alignment)
	{
		ctx.wanted_chr = chr_id;
	}

	void sample_names_from(std::string_view line)                     // the #CHROM line
	{
		field_cursor fc(line, '\t');
		std::string_view f;
		for (unsigned i(0); fc.next(f); ++i) if (i >= 9) vcf_sample_names.emplace_back(f);
	}

	void header_done()
	{
		ctx.n_samples = vcf_sample_names.size();
		ctx.copy_begin.assign(ctx.n_samples + 1, 0);
	}

	// A body line before the first record is known (1-based lineno): true when it is that record, and the layout is fixed.
	bool first_record(std::string_view line, u64 lineno)
	{
		if (!line.empty() && '\r' == line.back()) line.remove_suffix(1);
		if (line.empty() || '#' == line.front()) return false;
		field_cursor fc(line, '\t');
		std::string_view f, format;
		if (!fc.next(f)) return false;
		if (f != ctx.wanted_chr) return false;
		for (int i(1); i < 8; ++i) if (!fc.next(f)) bad(lineno, "fewer than 8 columns");
		if (!fc.next(format)) bad(lineno, "variant does not have a genotype");
		std::size_t gt_index(SIZE_MAX);
		{
			field_cursor ff(format, ':');
			std::string_view x;
			for (std::size_t i(0); ff.next(x); ++i) if (x == "GT") { gt_index = i; break; }
			if (SIZE_MAX == gt_index) bad(lineno, "variant does not have a genotype");
		}
		std::vector<std::string> names;
		std::vector<u32> ploidies;
		u32 row(0);
		std::size_t s(0);
		for (std::string_view field; fc.next(field); ++s) {
			if (s >= ctx.n_samples) bad(lineno, "more sample columns than in the header");
			std::string_view gt;
			{
				field_cursor sf(field, ':');
				std::size_t i(0);
				bool found(false);
				for (std::string_view x; sf.next(x); ++i) if (i == gt_index) { gt = x; found = true; break; }
				if (!found) bad(lineno, "sample without GT");
			}
			u32 ploidy(1);
			for (char const c : gt) if ('|' == c || '/' == c) ++ploidy;
			u32 kept(0);
			for (u32 c(0); c < ploidy; ++c) {
				bool const inc(delegate.should_include(vcf_sample_names[s], c));       // :231
				ctx.row_lookup.push_back(inc ? std::int32_t(row) : -1);
				if (inc) { ++row; ++kept; }
			}
			ctx.copy_begin[s + 1] = u32(ctx.row_lookup.size());
			if (kept) { names.push_back(vcf_sample_names[s]); ploidies.push_back(kept); }   // samples with no included copy are dropped (:250-273)
		}
		if (s != ctx.n_samples) bad(lineno, "sample column count differs from the header");
		builder.begin(std::move(names), ploidies);
		ctx.n_rows = row;
		ctx.words_per_column = graph.paths_by_edge_and_chrom_copy.words_per_column();
		return true;
	}

	// No record on the requested chromosome: the reference leaves ploidy_csum empty and then reads it
	// out of bounds (hard part 10).  Here: no samples, REF only.
	void finish_without_records(u64 other_records)
	{
		builder.begin({}, {});
		stats.chr_id_mismatches += other_records;
		builder.finish(ref_seq.size());
	}

	void begin_merge(u64 lines_before)
	{
		lineno_base = lines_before;
		var_idx = 0;
		for (std::size_t smp(0); smp < ctx.n_samples; ++smp)
			for (u32 c(ctx.copy_begin[smp]); c < ctx.copy_begin[smp + 1]; ++c)
				if (ctx.row_lookup[c] >= 0) {
					if (row_origin.size() <= std::size_t(ctx.row_lookup[c])) row_origin.resize(std::size_t(ctx.row_lookup[c]) + 1);
					row_origin[std::size_t(ctx.row_lookup[c])] = {u32(smp), c - ctx.copy_begin[smp]};
				}
		reaches.assign(ctx.n_rows, 0);
	}

	// The merge stage.  Per chunk, in file order: the records go into the builder one by one -- nodes, edges, targets: cheap --,
	// the chunk's slice of the path matrix is copied into place, and every chromosome copy's first ALT of the chunk is checked
	// against where the copy's last ALT before the chunk reached (the overlap check, variant_graph.cc:408-418, across the chunk
	// boundary; inside the chunk the parser has made it).  Overlaps are reported in the reference's order: record by record, copy by copy.
	// Returns false when the delegate stopped the build at a REF mismatch (the graph is finished then).
	bool merge(parsed_chunk &chunk)
	{
		auto const now([] { return std::chrono::steady_clock::now(); });
		auto const since([&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); });
		auto const t1(now());
		// records parsed before an error are still merged first, so errors surface in file order
		u64 const first_edge(graph.edge_count());
		std::size_t n_merged(0);
		parsed_record const *stopped_at(nullptr);
		for (auto const &rec : chunk.records) {
			++stats.handled_variants;
			u64 const this_var(var_idx + rec.data_line_in_chunk);
			// the reference's order: the position check (variant_graph.cc:293-297) comes before the REF comparison (:307-314)
			if (builder.would_go_back(rec.ref_pos))
				throw std::runtime_error("variant " + std::to_string(this_var) + " has non-increasing position");
			{                                                                            // :307-314
				std::string_view const expected(rec.ref_pos <= ref_sv.size() ? ref_sv.substr(rec.ref_pos, rec.ref.size()) : std::string_view{});
				if (rec.ref != expected && !delegate.ref_column_mismatch(this_var, rec.ref_pos, rec.ref, expected)) { stopped_at = &rec; break; }
			}
			if (!builder.add_record(rec.ref_pos, rec.ref.size(), chunk.alts.data() + rec.alt_begin, rec.n_alts))
				throw std::runtime_error("variant " + std::to_string(this_var) + " has non-increasing position");   // :293-297
			++n_merged;
		}
		t_records += since(t1);
		auto const t2(now());
		{
			// the merged records' columns of the chunk's slice (all of them unless the build stops inside the chunk)
			u64 const n_columns(n_merged < chunk.records.size() ? chunk.records[n_merged].first_column : chunk.n_columns);
			if (graph.edge_count() - first_edge != n_columns) throw std::logic_error("VCF reader: the builder made other edges than the parser counted");
			auto &m(graph.paths_by_edge_and_chrom_copy);
			// (no chromosome copy included -- every sample excluded: the matrix has no rows, graph_builder grows no columns for it,
			// and there is nothing to copy; the edge count above is still checked)
			if (n_columns && ctx.words_per_column) {
				if (m.cols < first_edge + n_columns || m.words_per_column() != ctx.words_per_column) throw std::logic_error("VCF reader: the path matrix is not what the parser filled its slice for");
				std::memcpy(m.words.data() + first_edge * ctx.words_per_column, chunk.bits.data(), n_columns * ctx.words_per_column * sizeof(u64));
			}
			// overlaps: the parser's (inside the chunk) and, here, every copy's first ALT of the chunk against the chunks before
			u64 const n_inside(n_merged < chunk.records.size() ? chunk.records[n_merged].overlap_begin : chunk.overlaps.size());
			reported.assign(chunk.overlaps.begin(), chunk.overlaps.begin() + std::ptrdiff_t(n_inside));
			for (u64 row(0); row < ctx.n_rows; ++row) {
				u32 const r(chunk.first_record[row]);
				if (kNoRecord == r || r >= n_merged) continue;
				if (chunk.records[r].ref_pos < reaches[row]) reported.push_back({r, u32(row), chunk.first_alt[row]});
				reaches[row] = chunk.last_target[row];
			}
			if (reported.size() > n_inside) {
				auto const before([](chunk_overlap const &a, chunk_overlap const &b) { return a.record != b.record ? a.record < b.record : a.row < b.row; });
				std::sort(reported.begin() + std::ptrdiff_t(n_inside), reported.end(), before);
				std::inplace_merge(reported.begin(), reported.begin() + std::ptrdiff_t(n_inside), reported.end(), [](chunk_overlap const &a, chunk_overlap const &b) { return a.record != b.record ? a.record < b.record : a.row < b.row; });
			}
			for (auto const &o : reported)
				delegate.report_overlapping_alternative(lineno_base + chunk.records[o.record].line_in_chunk, chunk.records[o.record].ref_pos, chunk.records[o.record].id,
					vcf_sample_names[row_origin[o.row].first], row_origin[o.row].second, o.alt_number);
		}
		t_genotypes += since(t2);
		if (stopped_at) {
			// the reference stops parsing here (variant_graph.cc:312-313) and still adds the sink node (:437-451); the
			// records of other chromosomes it had passed by then have been counted (:203-207)
			stats.chr_id_mismatches += stopped_at->chr_mismatches_before;
			builder.add_record_node_only(stopped_at->ref_pos);
			builder.finish(ref_seq.size());
			return false;
		}
		if (!chunk.error.empty()) bad(lineno_base + chunk.error_line, chunk.error.c_str());
		stats.chr_id_mismatches += chunk.chr_mismatches;
		lineno_base += chunk.n_lines;
		var_idx += chunk.n_data_lines;
		return true;
	}

	void finish() { builder.finish(ref_seq.size()); }                 // :437-451
};

} // namespace


void build_variant_graph(
	sequence_type const &ref_seq, char const *variants_path, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, unsigned threads, u64 path_alignment)
{
	mapped_file const file(variants_path);
	build_variant_graph(ref_seq, std::string_view(file.data, file.size), chr_id, graph, stats, delegate, threads, path_alignment);
}


void build_variant_graph(
	sequence_type const &ref_seq, std::string_view text, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, unsigned threads, u64 path_alignment)
{
	graph_assembly as(ref_seq, chr_id, graph, stats, delegate, path_alignment);
	parse_context const &ctx(as.ctx);

	// ---- header, then the first record on the requested chromosome: it fixes ploidy and inclusion (:215-288) ----
	std::size_t body_begin(0);
	u64 header_lines(0);
	{
		std::size_t pos(0);
		while (pos < text.size()) {
			std::size_t eol(text.find('\n', pos));
			if (std::string_view::npos == eol) eol = text.size();
			std::string_view line(text.substr(pos, eol - pos));
			if (!line.empty() && '\r' == line.back()) line.remove_suffix(1);
			if (!line.empty() && '#' != line.front()) break;
			if (line.substr(0, 6) == "#CHROM") as.sample_names_from(line);
			pos = eol + 1;
			++header_lines;
		}
		body_begin = std::min(pos, text.size());
	}
	as.header_done();
	bool have_first(false);
	{
		std::size_t pos(body_begin);
		u64 lineno(header_lines);
		while (pos < text.size() && !have_first) {
			std::size_t eol(text.find('\n', pos));
			if (std::string_view::npos == eol) eol = text.size();
			std::string_view const line(text.substr(pos, eol - pos));
			pos = eol + 1;
			++lineno;
			have_first = as.first_record(line, lineno);
		}
	}
	if (!have_first) {
		u64 others(0);
		for (std::size_t pos(body_begin); pos < text.size();) {
			std::size_t eol(text.find('\n', pos));
			if (std::string_view::npos == eol) eol = text.size();
			if (eol > pos && '#' != text[pos]) ++others;
			pos = eol + 1;
		}
		as.finish_without_records(others);
		return;
	}

	// about one ALT edge per line of the size of the first record's (a hint for the path matrix's allocation, nothing more)
	{
		std::size_t const first_eol(text.find('\n', body_begin));
		std::size_t const line_bytes(std::max<std::size_t>(16, (std::string_view::npos == first_eol ? text.size() : first_eol) - body_begin + 1));
		as.builder.expect_edges(u64(double(text.size() - body_begin) / double(line_bytes) * 1.1) + 1024);
	}

	// ---- chunks of whole lines, parsed by worker threads, merged in file order -------------------------------------
	if (0 == threads) threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
	std::size_t const target_chunk(std::size_t(8) << 20);
	std::vector<std::pair<std::size_t, std::size_t>> ranges;
	for (std::size_t b(body_begin); b < text.size();) {
		std::size_t e(std::min(text.size(), b + target_chunk));
		if (e < text.size()) {
			std::size_t const nl(text.find('\n', e));
			e = (std::string_view::npos == nl) ? text.size() : nl + 1;
		}
		ranges.emplace_back(b, e);
		b = e;
	}

	std::size_t const n_chunks(ranges.size());
	std::vector<parsed_chunk> chunks(n_chunks);
	std::vector<char> ready(n_chunks, 0);
	std::mutex mutex;
	std::condition_variable cv_ready, cv_window;
	std::size_t next_chunk(0), consumed(0);
	std::size_t const window(std::max<std::size_t>(2, 2 * threads));
	bool abort_workers(false);
	std::vector<parsed_chunk> spare_chunks;                           // (under `mutex`) consumed chunks: their vectors' pages are there already

	auto const worker([&] {
		for (;;) {
			std::size_t idx;
			{
				std::unique_lock<std::mutex> lock(mutex);
				cv_window.wait(lock, [&] { return abort_workers || next_chunk >= n_chunks || next_chunk < consumed + window; });
				if (abort_workers || next_chunk >= n_chunks) return;
				idx = next_chunk++;
			}
			{
				// (the vectors of a chunk that has been merged: their pages are there already; fresh ones of this size come from
				// mmap every time and cost a fault per page)
				std::lock_guard<std::mutex> lock(mutex);
				if (!spare_chunks.empty()) { chunks[idx] = std::move(spare_chunks.back()); spare_chunks.pop_back(); }
			}
			parse_chunk(text.substr(ranges[idx].first, ranges[idx].second - ranges[idx].first), ctx, chunks[idx]);
			{
				std::lock_guard<std::mutex> lock(mutex);
				ready[idx] = 1;
			}
			cv_ready.notify_all();
		}
	});
	std::vector<std::thread> pool;
	if (threads > 1)
		for (unsigned t(0); t < std::min<std::size_t>(threads, n_chunks); ++t) pool.emplace_back(worker);
	struct joiner {
		std::vector<std::thread> &pool; std::mutex &mutex; std::condition_variable &cv; bool &abort_flag;
		~joiner()
		{
			{ std::lock_guard<std::mutex> lock(mutex); abort_flag = true; }
			cv.notify_all();
			for (auto &t : pool) t.join();
		}
	} const join_on_exit{pool, mutex, cv_window, abort_workers};

	as.begin_merge(header_lines);

	// V2M_READER_TIMING=1: where the merge stage's time went (waiting for parsed chunks / records into the builder / bits and overlaps), to stderr
	bool const timing(nullptr != std::getenv("V2M_READER_TIMING"));
	double t_wait(0);
	auto const now([] { return std::chrono::steady_clock::now(); });
	auto const since([&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); });
	struct report_timing {
		bool on; double const &w, &r, &g;
		~report_timing() { if (on) std::fprintf(stderr, "[vcf reader] merge stage: %.3f s waiting for parsed chunks, %.3f s records into the builder, %.3f s path bits and overlaps\n", w, r, g); }
	} const report{timing, t_wait, as.t_records, as.t_genotypes};

	for (std::size_t ci(0); ci < n_chunks; ++ci) {
		auto const t0(now());
		if (threads > 1) {
			std::unique_lock<std::mutex> lock(mutex);
			cv_ready.wait(lock, [&] { return 0 != ready[ci]; });
		} else {
			parse_chunk(text.substr(ranges[ci].first, ranges[ci].second - ranges[ci].first), ctx, chunks[ci]);
		}
		t_wait += since(t0);
		parsed_chunk &chunk(chunks[ci]);
		if (!as.merge(chunk)) return;
		if (threads > 1) {
			{
				std::lock_guard<std::mutex> lock(mutex);
				consumed = ci + 1;
				chunk.records.clear(); chunk.alts.clear(); chunk.n_lines = chunk.n_data_lines = chunk.chr_mismatches = 0;
				spare_chunks.emplace_back(std::move(chunk));
				chunk = parsed_chunk{};
			}
			cv_window.notify_all();
		}
		else chunk = parsed_chunk{};
	}
	as.finish();
}


// ---- the scanned path (readers.hh) ---------------------------------------------------------------------------------------------------

namespace {

// Column 1 of a line for the layout test: up to the first tab; without a tab the whole line less a final '\r'.
std::string_view first_column(std::string_view line)
{
	std::size_t const tab(line.find('\t'));
	if (std::string_view::npos != tab) return line.substr(0, tab);
	if (!line.empty() && '\r' == line.back()) line.remove_suffix(1);
	return line;
}

} // namespace


int scan_lines_host(std::string_view text, char const *wanted_chr, std::size_t slice_bytes, v2m_vcf_layout_fn layout, v2m_vcf_chunk_fn chunk, void *user)
{
	std::string_view const wanted(wanted_chr);
	if (0 == slice_bytes) slice_bytes = std::size_t(64) << 20;
	bool have_layout(false);
	v2m_vcf_layout lay{};
	u64 first_line(0);
	std::vector<v2m_vcf_line> lines;
	std::string heads;
	std::vector<u64> columns;
	u64 n_columns(0);                                                 // counted on their own: with words_per_column == 0 the columns have no words
	auto const flush([&]() -> int {
		if (lines.empty()) return V2M_OK;
		v2m_vcf_chunk c{};
		c.first_line = first_line;
		c.n_lines = lines.size();
		c.lines = lines.data();
		c.heads = heads.data();
		c.head_bytes = heads.size();
		c.columns = columns.data();
		c.n_columns = n_columns;
		c.words_per_column = have_layout ? lay.words_per_column : 0;
		if (0 != chunk(user, &c)) return V2M_ERR_SINK;
		first_line += lines.size();
		lines.clear();
		heads.clear();
		columns.clear();
		n_columns = 0;
		return V2M_OK;
	});
	// slices as v2m_vcf_scan cuts plain text: the line the previous slice ended in, then as many new bytes as the slot still holds
	std::size_t const slot(std::max<std::size_t>(16, std::min<std::size_t>(slice_bytes, std::size_t(256) << 20)));
	for (std::size_t pos(0), taken(0); pos < text.size();) {
		lines.clear();
		heads.clear();
		columns.clear();
		n_columns = 0;
		std::size_t const carry(taken - pos), fresh(std::min(text.size() - taken, slot - std::min(slot, carry)));
		taken += fresh;
		bool const last(taken == text.size());
		if (!last && (0 == fresh || (taken - pos >= slot && std::string_view::npos == text.substr(pos, taken - pos).find('\n')))) return V2M_ERR_UNSUPPORTED;
		while (pos < taken) {
			std::size_t eol(text.substr(0, taken).find('\n', pos));
			if (std::string_view::npos == eol) {
				if (!last) break;                                               // carried into the next slice
				eol = text.size();
			}
			std::string_view const line(text.substr(pos, eol - pos));
			pos = eol + 1;

			v2m_vcf_line r{};
			r.head_offset = std::uint32_t(heads.size());
			r.column_begin = n_columns;
			auto const whole([&] { r.head_length = std::uint32_t(line.size()); heads.append(line); });
			if (line.empty() || '#' == line.front()) {
				r.kind = 0;
				if (line.substr(0, 6) == "#CHROM") whole();
				lines.push_back(r);
				continue;
			}
			std::size_t tabs[9];
			std::size_t n_tabs(0);
			for (std::size_t i(0); i < line.size() && n_tabs < 9; ++i) if ('\t' == line[i]) tabs[n_tabs++] = i;
			bool const on_chr(first_column(line) == wanted);
			if (on_chr && !have_layout) {
				// the lines before the layout line are a chunk of their own: the caller has seen the #CHROM line when `layout` runs
				if (!lines.empty()) {
					if (int const rc = flush()) return rc;
					r.head_offset = 0;
				}
				if (0 != layout(user, first_line, line.data(), line.size(), &lay)) return V2M_ERR_SINK;
				if (lay.n_rows > 32768 || lay.words_per_column > 512) return V2M_ERR_UNSUPPORTED;
				have_layout = true;
			}
			r.kind = 3;
			if (n_tabs < 7) { whole(); lines.push_back(r); continue; }
			if (!on_chr) { r.kind = 1; lines.push_back(r); continue; }
			bool ok('\r' != line.back() && 9 == n_tabs);
			if (ok) {
				std::string_view const format(line.substr(tabs[7] + 1, tabs[8] - tabs[7] - 1));
				ok = format == "GT" || format.substr(0, 3) == "GT:";
			}
			std::uint32_t n_alts(1);
			if (ok) {
				for (std::size_t i(tabs[3] + 1); i < tabs[4]; ++i) if (',' == line[i]) ++n_alts;
				ok = n_alts <= 8;
			}
			std::size_t const columns_before(columns.size());
			if (ok) {
				columns.resize(columns_before + n_alts * lay.words_per_column, 0);
				u64 *const cols(columns.data() + columns_before);
				// the sample columns: split at tabs, each one's GT subfield at '|' and '/'
				std::size_t sample(0), p(tabs[8] + 1);
				for (;; ++sample) {
					std::size_t field_end(line.find('\t', p));
					if (std::string_view::npos == field_end) field_end = line.size();
					if (sample >= lay.n_samples) { ok = false; break; }
					std::size_t gt_end(p);
					while (gt_end < field_end && ':' != line[gt_end]) ++gt_end;
					std::uint32_t const ploidy(lay.copy_begin[sample + 1] - lay.copy_begin[sample]);
					std::uint32_t c(0);
					for (std::size_t a(p); c < ploidy; ++c) {
						if (a > gt_end) { ok = false; break; }              // the token does not exist
						std::size_t b(a);
						while (b < gt_end && '|' != line[b] && '/' != line[b]) ++b;
						std::string_view const tok(line.substr(a, b - a));
						std::uint32_t allele(0);
						if (tok != ".") {
							if (tok.empty() || tok.size() > 3) { ok = false; break; }
							for (char const ch : tok) { if (ch < '0' || '9' < ch) { ok = false; break; } allele = 10 * allele + std::uint32_t(ch - '0'); }
							if (!ok || allele > n_alts) { ok = false; break; }
						}
						if (allele) {
							std::int32_t const row(lay.row_lookup[lay.copy_begin[sample] + c]);
							if (row >= 0) cols[(allele - 1) * lay.words_per_column + (std::uint32_t(row) >> 6)] |= u64(1) << (std::uint32_t(row) & 63);
						}
						a = b + 1;
					}
					if (!ok) break;
					if (field_end == line.size()) { ++sample; break; }
					p = field_end + 1;
				}
				ok = ok && sample == lay.n_samples;
			}
			if (ok) {
				r.kind = 2;
				r.n_alts = n_alts;
				r.head_length = std::uint32_t(tabs[8]);
				heads.append(line.substr(0, tabs[8]));
				n_columns += n_alts;
			} else {
				columns.resize(columns_before);
				whole();
			}
			lines.push_back(r);
		}
		if (int const rc = flush()) return rc;
	}
	return V2M_OK;
}


namespace {

// What the two callbacks of a scan do for build_variant_graph_scanned: the layout from the first record, and per chunk the assembler
// (a parsed_chunk from the scanned lines) and the merge stage, on the calling thread.  A chunk lies wholly before the layout line or
// wholly from it on.  Of the lines before it the text path's parser, which sees them with the layout in force, makes counts and at most
// one error ("fewer than 8 columns": such a line has fewer than 7 tabs); they are kept as that.
struct scanned_build {
	graph_assembly as;
	scan_statistics *scan_stats;
	u64 expected_bytes;
	bool have_layout{false}, stopped{false}, body_begun{false};
	u64 header_lines{0}, pre_lines{0}, pre_data_lines{0}, pre_mismatches{0}, pre_others{0}, pre_error_line{0};
	std::exception_ptr error;
	parsed_chunk parsed;
	double t_assemble{0};                                            // V2M_READER_TIMING: the assembler's share of the callbacks
	u64 chunks{0}, chunk_bytes{0};                                   // the chunks and what they brought to the host

	scanned_build(sequence_type const &ref, char const *chr_id, variant_graph &g, build_graph_statistics &st, build_graph_delegate &d, u64 path_alignment,
		scan_statistics *ss, u64 bytes) : as(ref, chr_id, g, st, d, path_alignment), scan_stats(ss), expected_bytes(bytes) {}

	static std::string_view strip_cr(std::string_view s) { if (!s.empty() && '\r' == s.back()) s.remove_suffix(1); return s; }

	int layout(u64 line_index, std::string_view line, v2m_vcf_layout *out)
	{
		try {
			as.header_done();
			if (!as.first_record(line, line_index + 1)) throw std::logic_error("VCF reader: the scan's layout line is not on the requested chromosome");
			have_layout = true;
			as.builder.expect_edges(u64(double(expected_bytes) / double(std::max<std::size_t>(16, line.size() + 1)) * 1.1) + 1024);
			as.begin_merge(header_lines);
			// (the text path finds this error when it merges its first chunk, after the first record has been accepted)
			if (pre_error_line) bad(header_lines + pre_error_line, "fewer than 8 columns");
			as.lineno_base += pre_lines;
			as.var_idx += pre_data_lines;
			as.stats.chr_id_mismatches += pre_mismatches;
			out->n_samples = std::uint32_t(as.ctx.n_samples);
			out->n_rows = std::uint32_t(as.ctx.n_rows);
			out->words_per_column = as.ctx.words_per_column;
			out->copy_begin = as.ctx.copy_begin.data();
			out->row_lookup = as.ctx.row_lookup.data();
			return 0;
		} catch (...) { error = std::current_exception(); return 1; }
	}

	void before_layout(v2m_vcf_chunk const &c)
	{
		for (u64 i(0); i < c.n_lines; ++i) {
			v2m_vcf_line const &l(c.lines[i]);
			std::string_view const head(strip_cr(std::string_view(c.heads + l.head_offset, l.head_length)));
			bool const blank(0 == l.kind || (3 == l.kind && head.empty()));   // empty, '#...' or "\r"
			if (!body_begun) {
				if (blank) {
					++header_lines;
					if (0 == l.kind && !head.empty()) as.sample_names_from(head);
					continue;
				}
				body_begun = true;
			}
			++pre_lines;
			if (0 != l.kind) ++pre_others;
			if (1 == l.kind) { ++pre_data_lines; ++pre_mismatches; }
			else if (!blank && !pre_error_line) pre_error_line = pre_lines;
		}
	}

	int chunk(v2m_vcf_chunk const &c)
	{
		try {
			if (scan_stats) for (u64 i(0); i < c.n_lines; ++i) { ++scan_stats->lines; if (3 == c.lines[i].kind) ++scan_stats->declined; }
			++chunks;
			chunk_bytes += c.n_lines * sizeof(v2m_vcf_line) + c.head_bytes + c.n_columns * c.words_per_column * sizeof(u64);
			if (!have_layout) { before_layout(c); return 0; }
			auto const t0(std::chrono::steady_clock::now());
			// the assembler: the chunk's lines into a parsed_chunk, as parse_chunk makes one from text
			parsed.records.clear(); parsed.alts.clear(); parsed.n_lines = parsed.n_data_lines = parsed.chr_mismatches = 0;
			parsed.error.clear(); parsed.error_line = 0;
			chunk_parser parser(as.ctx, parsed);
			try {
				for (u64 i(0); i < c.n_lines; ++i) {
					v2m_vcf_line const &l(c.lines[i]);
					std::string_view const head(c.heads + l.head_offset, l.head_length);
					switch (l.kind) {
						case 0: ++parsed.n_lines; break;
						case 1: ++parsed.n_lines; ++parsed.n_data_lines; ++parsed.chr_mismatches; break;
						case 2: parser.scanned_line(head, c.columns + l.column_begin * c.words_per_column, l.n_alts); break;
						default: parser.line(head); break;
					}
				}
			} catch (chunk_error const &e) {
				parser.failed(e);
			}
			t_assemble += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
			if (!as.merge(parsed)) stopped = true;
			return stopped ? 1 : 0;                                      // (stopped at a REF mismatch: the scan ends here, as the text path does)
		} catch (...) { error = std::current_exception(); return 1; }
	}
};

} // namespace


void build_variant_graph_scanned(
	sequence_type const &ref_seq, line_scanner const &scanner, u64 expected_text_bytes, char const *chr_id,
	variant_graph &graph, build_graph_statistics &stats, build_graph_delegate &delegate, scan_statistics *scan_stats, u64 path_alignment)
{
	scanned_build sb(ref_seq, chr_id, graph, stats, delegate, path_alignment, scan_stats, expected_text_bytes);
	// V2M_READER_TIMING=1: where the scanned build's time went (the scanner itself / the assembler / the merge stage's two parts), to stderr
	struct report_timing {
		bool on; std::chrono::steady_clock::time_point t0; scanned_build const &sb;
		~report_timing()
		{
			if (!on) return;
			double const all(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
			std::fprintf(stderr, "[vcf reader] scanned build: %.3f s in all; %.3f s in the scanner, %.3f s assembling chunks, %.3f s records into the builder, "
				"%.3f s path bits and overlaps; %llu chunks, %llu bytes to the host\n", all, all - sb.t_assemble - sb.as.t_records - sb.as.t_genotypes, sb.t_assemble,
				sb.as.t_records, sb.as.t_genotypes, (unsigned long long) sb.chunks, (unsigned long long) sb.chunk_bytes);
		}
	} const report{nullptr != std::getenv("V2M_READER_TIMING"), std::chrono::steady_clock::now(), sb};
	int const rc(scanner(chr_id,
		[](void *user, uint64_t line_index, char const *line, uint64_t length, v2m_vcf_layout *out) -> int {
			return static_cast<scanned_build *>(user)->layout(line_index, std::string_view(line, length), out);
		},
		[](void *user, v2m_vcf_chunk const *c) -> int { return static_cast<scanned_build *>(user)->chunk(*c); }, &sb));
	if (sb.error) std::rethrow_exception(sb.error);
	if (sb.stopped) return;                                          // (the scanner's code is the stopped callback's)
	if (V2M_OK != rc) throw scan_failed(rc);
	if (!sb.have_layout) { sb.as.header_done(); sb.as.finish_without_records(sb.pre_others); return; }
	sb.as.finish();
}

} // namespace v2m::host
