#include "output.hh"
#include "../nj_support.hpp"
#include <cstdlib>
#include <cstdio>
#include <chrono>

#include <fcntl.h>
#include <sys/uio.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <algorithm>
#include <cctype>
#include <cmath>
#include <limits>
#include <map>
#include <set>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <exception>
#include <mutex>
#include <fstream>
#include <stdexcept>
#include <streambuf>
#include <iostream>
#include <thread>

namespace v2m::host {

output::output(gpu_context &gpu, char const *pipe_cmd, char const *chromosome_id, bool should_output_reference, bool should_output_unaligned, output_delegate &delegate):
	m_gpu(gpu), m_pipe_cmd(pipe_cmd), m_chromosome_id(chromosome_id), m_delegate(&delegate),
	m_should_output_reference(should_output_reference), m_should_output_unaligned(should_output_unaligned)
{
}


namespace {
	// --pipe (output.cc:26-38,49-68): `command dst_name` as a child process that reads the sequences from its standard
	// input instead of us writing the file.  libbio::subprocess<STDIN> with KEEP_STDERR there: the child's stderr is
	// ours; its stdout goes to /dev/null here (libbio is not part of the reference tree, so this detail is unpinned).
	class pipe_process {
	public:
		pipe_process(char const *command, char const *dst_name)
		{
			int in[2], status[2];
			if (0 != ::pipe2(in, O_CLOEXEC)) fail_errno("pipe");
			if (0 != ::pipe2(status, O_CLOEXEC)) { int const e(errno); ::close(in[0]); ::close(in[1]); errno = e; fail_errno("pipe"); }
			m_pid = ::fork();
			if (m_pid < 0) { int const e(errno); ::close(in[0]); ::close(in[1]); ::close(status[0]); ::close(status[1]); errno = e; fail_errno("fork"); }
			if (0 == m_pid) {
				// child: only async-signal-safe calls from here on
				if (::dup2(in[0], STDIN_FILENO) >= 0) {
					int const null_fd(::open("/dev/null", O_WRONLY));
					if (null_fd >= 0) { ::dup2(null_fd, STDOUT_FILENO); ::close(null_fd); }
					char *const argv[] = {const_cast<char *>(command), const_cast<char *>(dst_name), nullptr};
					::execvp(command, argv);
				}
				int const e(errno);
				(void) !::write(status[1], &e, sizeof(e));
				::_exit(127);
			}
			::close(in[0]);
			::close(status[1]);
			m_fd = in[1];
			int child_errno(0);
			ssize_t got;
			do { got = ::read(status[0], &child_errno, sizeof(child_errno)); } while (got < 0 && EINTR == errno);
			::close(status[0]);
			if (got > 0) {                                                  // exec failed (main.cc:333-338)
				::close(m_fd);
				m_fd = -1;
				int st;
				::waitpid(m_pid, &st, 0);
				throw std::runtime_error(std::string("Unable to execute subprocess. ") + command + ": " + std::strerror(child_errno));
			}
		}

		pipe_process(pipe_process const &) = delete;
		pipe_process &operator=(pipe_process const &) = delete;

		~pipe_process()
		{
			if (m_fd >= 0) ::close(m_fd);
			if (m_pid > 0 && !m_waited) { int st; ::waitpid(m_pid, &st, 0); }
		}

		int fd() const { return m_fd; }

		// Close the child's standard input and wait for it; anything but exit(0) is an error (main.cc:341-367).
		void finish()
		{
			::close(m_fd);
			m_fd = -1;
			int st(0);
			pid_t r;
			do { r = ::waitpid(m_pid, &st, 0); } while (r < 0 && EINTR == errno);
			m_waited = true;
			if (r == m_pid && WIFEXITED(st) && 0 == WEXITSTATUS(st)) return;
			std::string msg("Subprocess with PID " + std::to_string(m_pid) + " exited with status ");
			if (r != m_pid) msg += "0 (exiting reason not known)";
			else if (WIFSIGNALED(st)) msg += std::to_string(WTERMSIG(st)) + " (terminated by signal)";
			else if (WIFSTOPPED(st)) msg += std::to_string(WSTOPSIG(st)) + " (stopped by signal)";
			else msg += std::to_string(WEXITSTATUS(st));
			throw std::runtime_error(msg);
		}

	private:
		[[noreturn]] static void fail_errno(char const *what)
		{
			throw std::runtime_error(std::string("Unable to execute subprocess. ") + what + ": " + std::strerror(errno));
		}

		pid_t m_pid{-1};
		int m_fd{-1};
		bool m_waited{};
	};


	// std::ostream over a file descriptor (the reference opens a libbio::file_ostream on the child's stdin handle).
	class fd_streambuf final : public std::streambuf {
	public:
		explicit fd_streambuf(int fd) : m_fd(fd), m_buffer(1u << 20) { setp(m_buffer.data(), m_buffer.data() + m_buffer.size()); }
		~fd_streambuf() override { sync(); }

	protected:
		int_type overflow(int_type ch) override
		{
			if (!flush_buffer()) return traits_type::eof();
			if (!traits_type::eq_int_type(ch, traits_type::eof())) { *pptr() = traits_type::to_char_type(ch); pbump(1); }
			return traits_type::not_eof(ch);
		}

		std::streamsize xsputn(char const *s, std::streamsize n) override
		{
			if (n < std::streamsize(m_buffer.size() / 4)) return std::streambuf::xsputn(s, n);
			if (!flush_buffer() || !write_all(s, std::size_t(n))) return 0;      // row bodies go straight from the pinned ring
			return n;
		}

		int sync() override { return flush_buffer() ? 0 : -1; }

	private:
		bool flush_buffer()
		{
			bool const ok(write_all(pbase(), std::size_t(pptr() - pbase())));
			setp(m_buffer.data(), m_buffer.data() + m_buffer.size());
			return ok;
		}

		bool write_all(char const *p, std::size_t n)
		{
			while (n) {
				ssize_t const w(::write(m_fd, p, n));
				if (w < 0) { if (EINTR == errno) continue; return false; }   // EPIPE when the child has gone away (SIGPIPE is ignored)
				p += w;
				n -= std::size_t(w);
			}
			return true;
		}

		int m_fd;
		std::vector<char> m_buffer;
	};
}


std::string output::prefixed(std::string const &name, char sep) const
{
	return m_chromosome_id ? std::string(m_chromosome_id) + sep + name : name;
}


namespace {
	// Lets the contexts' sink calls through in row order.  A context whose row is not due waits inside its sink call; the
	// library meanwhile keeps filling that context's other pinned slot, so the wait costs nothing but the turn itself.
	struct turnstile {
		std::mutex mutex;
		std::condition_variable turn;
		std::uint64_t next_row{};
		bool failed{};
	};

	struct turn_state {
		turnstile *gate;
		std::vector<std::uint64_t> const *global_row;   // of each row of this context's batch
		v2m_sink_fn sink;
		void *user;
	};

	int turn_sink(void *user, uint64_t row, char const *bytes, uint64_t length)
	{
		auto &st(*static_cast<turn_state *>(user));
		std::uint64_t const global((*st.global_row)[row]);
		std::unique_lock<std::mutex> lock(st.gate->mutex);
		st.gate->turn.wait(lock, [&] { return st.gate->failed || st.gate->next_row == global; });
		if (st.gate->failed) return 1;
		int const rc(st.sink(st.user, global, bytes, length));   // (under the lock: one writer at a time, in order)
		if (rc) st.gate->failed = true; else ++st.gate->next_row;
		lock.unlock();
		st.gate->turn.notify_all();
		return rc;
	}
}


// splice() over several contexts that hold the chromosome copies dealt round-robin (set_copy_interleave): the sink sees the
// rows in the batch's order, exactly as from one context.
void output::splice_in_turns(row_set const &rows, v2m_sink_fn sink, void *user, std::uint32_t extra_flags)
{
	if (rows.any_cuts) throw std::runtime_error("rows that switch copies need the whole path matrix on their GPU");
	std::vector<gpu_context *> gpus{&m_gpu};
	gpus.insert(gpus.end(), m_more_gpus.begin(), m_more_gpus.end());
	std::size_t const g(gpus.size());
	if (m_copy_interleave.world != g) throw std::runtime_error("the copy interleave was made for another number of GPU contexts");
	std::vector<std::vector<std::uint32_t>> local_copy(g);
	std::vector<std::vector<std::uint64_t>> global_row(g);
	for (std::uint64_t i(0); i < rows.copy_index.size(); ++i) {
		std::uint32_t const c(rows.copy_index[i]);
		bool const is_ref(V2M_PLOIDY_MAX == c);
		std::size_t const k(is_ref ? 0 : m_copy_interleave.owner(c));          // the REF row needs no path bits: first context
		local_copy[k].push_back(is_ref ? c : std::uint32_t(m_copy_interleave.local(c)));
		global_row[k].push_back(i);
	}
	turnstile gate;
	std::vector<std::exception_ptr> errors(g);
	std::vector<std::thread> threads;
	for (std::size_t k(0); k < g; ++k) {
		threads.emplace_back([&, k] {
			try {
				if (local_copy[k].empty()) return;
				v2m_row_batch batch{};
				batch.n_rows = local_copy[k].size();
				batch.copy_index = local_copy[k].data();
				turn_state st{&gate, &global_row[k], sink, user};
				gpus[k]->check(v2m_splice_rows(gpus[k]->get(), &batch, (m_should_output_unaligned ? V2M_SPLICE_UNALIGNED : 0u) | extra_flags, turn_sink, &st));
			} catch (...) {
				errors[k] = std::current_exception();
				{ std::lock_guard<std::mutex> const lock(gate.mutex); gate.failed = true; }   // nobody waits for this context's rows any longer
				gate.turn.notify_all();
			}
		});
	}
	for (auto &t : threads) t.join();
	// the first error in context order that is not just "my sink was told to stop"
	for (auto const &e : errors) {
		if (!e) continue;
		try { std::rethrow_exception(e); }
		catch (gpu_error const &ge) { if (V2M_ERR_SINK != ge.code) throw; }
	}
	for (auto const &e : errors) if (e) std::rethrow_exception(e);
}


void output::splice(row_set const &rows, v2m_sink_fn sink, void *user, std::uint32_t extra_flags)
{
	if (m_interleaved && !m_more_gpus.empty()) { splice_in_turns(rows, sink, user, extra_flags); return; }
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	std::vector<std::uint32_t> rebased;
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) {       // the first context's matrix starts at another copy
		rebased = rebased_copies(rows, 0, rows.copy_index.size(), m_copy_shards.front());
		batch.copy_index = rebased.data();
	}
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	m_gpu.check(v2m_splice_rows(m_gpu.get(), &batch, (m_should_output_unaligned ? V2M_SPLICE_UNALIGNED : 0u) | extra_flags, sink, user));
}


// Copy indices of rows [first, last) relative to the shard that holds them.
std::vector<std::uint32_t> output::rebased_copies(row_set const &rows, std::uint64_t first, std::uint64_t last, copy_shard shard)
{
	if (rows.any_cuts) throw std::runtime_error("rows that switch copies need the whole path matrix on their GPU");
	std::vector<std::uint32_t> out(rows.copy_index.begin() + first, rows.copy_index.begin() + last);
	for (auto &c : out) {
		if (V2M_PLOIDY_MAX == c) continue;
		if (c < shard.first || c >= shard.end) throw std::runtime_error("row of chromosome copy " + std::to_string(c) + " was given to a GPU that does not hold it");
		c -= std::uint32_t(shard.first);
	}
	return out;
}


namespace {
	struct a2m_state { std::ostream *stream; std::vector<std::string> const *ids; output_delegate *delegate; bool bgzf; std::string text; std::vector<char> framed; };

	// `n` bytes of text as stored BGZF members (v2m_bgzf_frame_stored; n = 0: the EOF member)
	void write_bgzf_stored(std::ostream &os, char const *bytes, std::size_t n, std::vector<char> &buf)
	{
		buf.resize(v2m_bgzf_bound(n));
		std::uint64_t written(0);
		if (V2M_OK != v2m_bgzf_frame_stored(bytes, n, buf.data(), buf.size(), &written)) throw std::runtime_error("v2m_bgzf_frame_stored failed");
		os.write(buf.data(), std::streamsize(written));
	}

	int a2m_sink(void *user, uint64_t row, char const *bytes, uint64_t length)
	{
		auto &st(*static_cast<a2m_state *>(user));
		if (st.bgzf) {                                                     // bytes = the body's BGZF members
			st.text.assign(1, '>');
			st.text += (*st.ids)[row];
			st.text += '\n';
			write_bgzf_stored(*st.stream, st.text.data(), st.text.size(), st.framed);
			st.stream->write(bytes, std::streamsize(length));
			write_bgzf_stored(*st.stream, "\n", 1, st.framed);
			st.delegate->handled_sequences(u32(1 + row));
			return st.stream->good() ? 0 : 1;
		}
		*st.stream << '>' << (*st.ids)[row] << '\n';                       // sequence_writer.cc:35-36
		st.stream->write(bytes, std::streamsize(length));
		*st.stream << '\n';                                                // haplotype_output.cc:57,76
		st.delegate->handled_sequences(u32(1 + row));                      // haplotype_output.cc:58,78-79
		return st.stream->good() ? 0 : 1;
	}

	struct separate_state { std::vector<std::string> const *names; char const *pipe_cmd; std::exception_ptr error; };

	// output_sequence_file always passes dst_name as the FASTA identifier, whatever should_include_fasta_header says
	// (output.cc:36,42), and no newline follows the body.
	void write_sequence_file(std::ostream &os, std::string const &name, char const *bytes, uint64_t length)
	{
		os << '>' << name << '\n';
		os.write(bytes, std::streamsize(length));
		os.flush();
	}

	int separate_sink(void *user, uint64_t row, char const *bytes, uint64_t length)
	{
		auto &st(*static_cast<separate_state *>(user));
		auto const &name((*st.names)[row]);
		if (st.pipe_cmd) {                                                  // output.cc:26-38
			try {
				pipe_process proc(st.pipe_cmd, name.c_str());
				bool good;
				{
					fd_streambuf buf(proc.fd());
					std::ostream os(&buf);
					write_sequence_file(os, name, bytes, length);
					good = os.good();
				}
				proc.finish();                                                  // throws if the child did not exit(0)
				if (!good) throw std::runtime_error("error while writing to the subprocess for " + name);
			} catch (...) {
				st.error = std::current_exception();
				return 1;
			}
			return 0;
		}
		std::ofstream os(name, std::ios::binary | std::ios::trunc);
		if (!os) return 1;
		write_sequence_file(os, name, bytes, length);
		return os.good() ? 0 : 1;
	}
}


namespace {
	// Writer threads behind a v2m_hold_sink_fn (v2m_splice_rows_held): the sink queues a row and returns, a writer writes the row's file from the
	// library's pinned slot and only then gives the row back.  One writer on one file moves 6-11 GB/s through the page cache, the link delivers
	// 56: a file per sequence scales with writers (profiles/r04/e2e_config2_file_destinations.txt), and with rows that may be kept ONE GPU
	// context is enough to feed them all.
	class row_writer_pool {
	public:
		typedef bool (*write_fn)(void *user, std::uint64_t row, char const *bytes, std::uint64_t length);

		row_writer_pool(unsigned n_threads, write_fn write, void *user) : m_write(write), m_user(user)
		{
			for (unsigned i(0); i < std::max(1u, n_threads); ++i) m_threads.emplace_back([this] { work(); });
		}

		~row_writer_pool() { finish(); }

		// the v2m_hold_sink_fn: `user` is the pool
		static int sink(void *user, uint64_t row, char const *bytes, uint64_t length, v2m_row_hold *hold)
		{
			auto &self(*static_cast<row_writer_pool *>(user));
			{
				std::lock_guard<std::mutex> const lock(self.m_mutex);
				if (self.m_failed) return 1;                                    // not accepted: the library ends the call
				self.m_jobs.push_back({row, bytes, length, hold});
			}
			self.m_wake.notify_one();
			return 0;
		}

		// every queued row written (or dropped after a failure) and released; false if a write failed
		bool finish()
		{
			{
				std::lock_guard<std::mutex> const lock(m_mutex);
				m_stopping = true;
			}
			m_wake.notify_all();
			for (auto &t : m_threads) t.join();
			m_threads.clear();
			return !m_failed;
		}

	private:
		struct job { std::uint64_t row; char const *bytes; std::uint64_t length; v2m_row_hold *hold; };

		void work()
		{
			for (;;) {
				job j;
				bool write;
				{
					std::unique_lock<std::mutex> lock(m_mutex);
					m_wake.wait(lock, [&] { return m_stopping || !m_jobs.empty(); });
					if (m_jobs.empty()) return;
					j = m_jobs.front();
					m_jobs.pop_front();
					write = !m_failed;
				}
				bool const ok(!write || m_write(m_user, j.row, j.bytes, j.length));
				v2m_row_release(j.hold);                                            // whatever happened to the file: the slot is the library's
				if (!ok) { std::lock_guard<std::mutex> const lock(m_mutex); m_failed = true; }
			}
		}

		write_fn m_write;
		void *m_user;
		std::mutex m_mutex;
		std::condition_variable m_wake;
		std::deque<job> m_jobs;
		std::vector<std::thread> m_threads;
		bool m_stopping{}, m_failed{};
	};

	unsigned env_count(char const *name, unsigned fallback, unsigned lo, unsigned hi)
	{
		char const *const e(std::getenv(name));
		long const v((e && *e) ? std::strtol(e, nullptr, 10) : 0);
		return unsigned(std::min<long>(hi, std::max<long>(lo, v > 0 ? v : long(fallback))));
	}

	struct held_turn_state { std::vector<std::uint64_t> const *global_row; v2m_hold_sink_fn sink; void *user; };

	int held_turn_sink(void *user, uint64_t row, char const *bytes, uint64_t length, v2m_row_hold *hold)
	{
		auto const &st(*static_cast<held_turn_state *>(user));
		return st.sink(st.user, (*st.global_row)[row], bytes, length, hold);
	}
}


// splice() for rows that need no order among themselves and a sink that keeps them for a while (v2m_splice_rows_held): one call per context,
// each on its own thread when there are several; the sink sees the batch's row indices.
void output::splice_held(row_set const &rows, v2m_hold_sink_fn sink, void *user)
{
	unsigned const n_slots(env_count("V2M_HELD_SLOTS", 4, 2, 64));
	std::uint32_t const flags(m_should_output_unaligned ? V2M_SPLICE_UNALIGNED : 0u);
	if (!(m_interleaved && !m_more_gpus.empty())) {
		v2m_row_batch batch{};
		batch.n_rows = rows.copy_index.size();
		batch.copy_index = rows.copy_index.data();
		std::vector<std::uint32_t> rebased;
		if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) {
			rebased = rebased_copies(rows, 0, rows.copy_index.size(), m_copy_shards.front());
			batch.copy_index = rebased.data();
		}
		if (rows.any_cuts) {
			batch.cut_offsets = rows.cut_offsets.data();
			batch.cut_nodes = rows.cut_nodes.data();
			batch.cut_copies = rows.cut_copies.data();
		}
		m_gpu.check(v2m_splice_rows_held(m_gpu.get(), &batch, flags, n_slots, sink, user));
		return;
	}
	if (rows.any_cuts) throw std::runtime_error("rows that switch copies need the whole path matrix on their GPU");
	std::vector<gpu_context *> gpus{&m_gpu};
	gpus.insert(gpus.end(), m_more_gpus.begin(), m_more_gpus.end());
	std::size_t const g(gpus.size());
	if (m_copy_interleave.world != g) throw std::runtime_error("the copy interleave was made for another number of GPU contexts");
	std::vector<std::vector<std::uint32_t>> local_copy(g);
	std::vector<std::vector<std::uint64_t>> global_row(g);
	for (std::uint64_t i(0); i < rows.copy_index.size(); ++i) {
		std::uint32_t const c(rows.copy_index[i]);
		bool const is_ref(V2M_PLOIDY_MAX == c);
		std::size_t const k(is_ref ? 0 : m_copy_interleave.owner(c));
		local_copy[k].push_back(is_ref ? c : std::uint32_t(m_copy_interleave.local(c)));
		global_row[k].push_back(i);
	}
	std::vector<std::exception_ptr> errors(g);
	std::vector<std::thread> threads;
	for (std::size_t k(0); k < g; ++k) {
		threads.emplace_back([&, k] {
			try {
				if (local_copy[k].empty()) return;
				v2m_row_batch batch{};
				batch.n_rows = local_copy[k].size();
				batch.copy_index = local_copy[k].data();
				held_turn_state st{&global_row[k], sink, user};
				gpus[k]->check(v2m_splice_rows_held(gpus[k]->get(), &batch, flags, n_slots, held_turn_sink, &st));
			} catch (...) {
				errors[k] = std::current_exception();
			}
		});
	}
	for (auto &t : threads) t.join();
	for (auto const &e : errors) {                                                      // the first error that is not just "my sink was told to stop"
		if (!e) continue;
		try { std::rethrow_exception(e); }
		catch (gpu_error const &ge) { if (V2M_ERR_SINK != ge.code) throw; }
	}
	for (auto const &e : errors) if (e) std::rethrow_exception(e);
}


void output::write_a2m(row_set const &rows, std::ostream &stream)
{
	a2m_state st{&stream, &rows.ids, m_delegate, m_bgzf, {}, {}};
	splice(rows, a2m_sink, &st, m_bgzf ? V2M_SPLICE_BGZF : 0u);
	if (m_bgzf) write_bgzf_stored(stream, nullptr, 0, st.framed);
}


void output::write_separate(row_set const &rows)
{
	separate_state st{&rows.ids, m_pipe_cmd, nullptr};
	if (!m_pipe_cmd) {
		// Files of their own need no order among themselves and no single writer: the rows stay in the library's pinned slots while a pool
		// of threads writes them out (V2M_WRITER_THREADS, default 8 in all), so that ONE context's link is fed by as many writers as it takes.
		// With several GPU contexts each one's thread delivers into the same pool.
		struct file_writer {
			static bool write(void *user, std::uint64_t row, char const *bytes, std::uint64_t length) { return 0 == separate_sink(user, row, bytes, length); }
		};
		row_writer_pool pool(env_count("V2M_WRITER_THREADS", 8, 1, 64), &file_writer::write, &st);
		std::exception_ptr error;
		try { splice_held(rows, &row_writer_pool::sink, &pool); } catch (...) { error = std::current_exception(); }
		bool const written(pool.finish());
		if (!written) throw std::runtime_error("error while writing a sequence file");      // the telling error, not "sink failed"
		if (error) std::rethrow_exception(error);
		return;
	}
	try {
		// Subprocesses (--pipe) are started one after the other, as the reference starts them (output.cc:26-38).
		splice(rows, separate_sink, &st);
	} catch (...) {
		if (st.error) std::rethrow_exception(st.error);                     // what went wrong with the subprocess, not "sink failed"
		throw;
	}
}


namespace {
	struct regions_state {
		std::vector<std::ofstream> *files;
		std::vector<std::uint64_t> const *slot_offset;
		std::vector<std::string> const *ids;
		output_delegate *delegate;          // told about the rows on the last pass only
	};

	int regions_sink(void *user, uint64_t row, char const *record, uint32_t const *lengths)
	{
		auto &st(*static_cast<regions_state *>(user));
		auto const &id((*st.ids)[row]);
		for (std::size_t k(0); k < st.files->size(); ++k) {
			auto &os((*st.files)[k]);
			os << '>' << id << '\n';                                           // as a2m_sink writes a row
			os.write(record + (*st.slot_offset)[k], std::streamsize(lengths[k]));
			os << '\n';
			if (!os.good()) return 1;
		}
		if (st.delegate) st.delegate->handled_sequences(u32(1 + row));
		return 0;
	}

	struct distinct_state {
		std::vector<std::ofstream> *files;
		std::vector<std::string> const *ids;
		std::vector<std::vector<std::uint64_t>> first_rows;   // per region: the first row of each class, in class order
		std::uint64_t bytes{};
	};

	int distinct_sink(void *user, uint64_t window, uint64_t class_index, uint64_t first_row, char const *bytes, uint64_t length)
	{
		auto &st(*static_cast<distinct_state *>(user));
		auto &os((*st.files)[window]);
		if (class_index != st.first_rows[window].size()) return 1;
		st.first_rows[window].push_back(first_row);
		os << '>' << (*st.ids)[first_row] << '\n';                             // the record regions_sink writes for that row
		os.write(bytes, std::streamsize(length));
		os << '\n';
		st.bytes += length;
		return os.good() ? 0 : 1;
	}
}


void output::output_regions(variant_graph const &graph, std::vector<output_region> const &regions, std::size_t regions_per_pass, bool distinct, bool verbose)
{
	row_set const rows(a2m_rows(graph));
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	std::vector<std::uint32_t> rebased;
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) {
		rebased = rebased_copies(rows, 0, rows.copy_index.size(), m_copy_shards.front());
		batch.copy_index = rebased.data();
	}
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	char const *const suffix(m_should_output_unaligned ? ".fa" : ".a2m");
	std::size_t const per_pass(std::max<std::size_t>(1, regions_per_pass));
	for (std::size_t first(0); first < regions.size(); first += per_pass) {
		std::size_t const n(std::min(per_pass, regions.size() - first));
		std::vector<std::uint64_t> begin(n), end(n), slot_offset(n);
		for (std::size_t k(0); k < n; ++k) { begin[k] = regions[first + k].col_begin; end[k] = regions[first + k].col_end; }
		std::uint64_t pitch(0);
		if (V2M_OK != v2m_window_set_layout(n, begin.data(), end.data(), slot_offset.data(), &pitch)) throw std::runtime_error(v2m_last_error(nullptr));
		m_gpu.check(v2m_set_window_set(m_gpu.get(), n, begin.data(), end.data()));
		std::vector<std::ofstream> files(n);
		for (std::size_t k(0); k < n; ++k) {
			std::string const name(regions[first + k].name + suffix);
			files[k].open(name, std::ios::binary | std::ios::trunc);
			if (!files[k]) throw std::runtime_error("unable to open " + name + " for writing");
		}
		if (distinct) {
			std::uint64_t const n_rows(batch.n_rows);
			std::vector<std::uint32_t> class_of(std::max<std::uint64_t>(1, n_rows * n)), n_classes(n);
			distinct_state st{&files, &rows.ids, std::vector<std::vector<std::uint64_t>>(n), 0};
			m_gpu.check(v2m_splice_window_set_distinct(m_gpu.get(), &batch, m_should_output_unaligned ? V2M_SPLICE_UNALIGNED : 0u, distinct_sink, &st, class_of.data(), n_classes.data()));
			std::uint64_t n_distinct(0);
			for (std::size_t k(0); k < n; ++k) {
				std::string const name(regions[first + k].name + ".classes.tsv");
				std::ofstream tsv(name, std::ios::binary | std::ios::trunc);
				if (!tsv) throw std::runtime_error("unable to open " + name + " for writing");
				for (std::uint64_t r(0); r < n_rows; ++r) {
					std::uint32_t const c(class_of[r * n + k]);
					tsv << rows.ids[r] << '\t' << rows.ids[st.first_rows[k].at(c)] << '\t' << c << '\n';
				}
				tsv.close();
				if (!tsv) throw std::runtime_error("error while writing " + name);
				n_distinct += n_classes[k];
			}
			if (verbose)
				std::cerr << "\n  regions " << first << ".." << first + n - 1 << ": " << n_rows * n << " pieces, " << n_distinct << " distinct pieces, " << st.bytes << " bytes over the link" << std::flush;
			if (m_delegate && first + n == regions.size()) m_delegate->handled_sequences(u32(n_rows));
		}
		else {
			regions_state st{&files, &slot_offset, &rows.ids, first + n == regions.size() ? m_delegate : nullptr};
			m_gpu.check(v2m_splice_window_set(m_gpu.get(), &batch, m_should_output_unaligned ? V2M_SPLICE_UNALIGNED : 0u, regions_sink, &st));
		}
		for (std::size_t k(0); k < n; ++k) {
			files[k].close();
			if (!files[k]) throw std::runtime_error("error while writing " + regions[first + k].name + suffix);
		}
	}
}


namespace {
	// One shard of an aligned A2M file: rows [first, first + n) of the batch, written at precomputed file offsets.
	struct shard_state {
		int fd;
		std::vector<std::string> const *ids;
		std::uint64_t const *offsets;      // file offset of each row of the whole batch
		std::uint64_t first;               // batch index of the shard's row 0
		std::mutex *one_writer;            // buffered writes into ONE file run under its inode lock anyway; several threads inside the kernel at
		                                   // once only fight over it (tmpfs, two writers: 20 GB in 5.4 s against 3.2 s for one; profiles/r04/
		                                   // e2e_config2_file_destinations.txt), so they take turns out here
	};

	int shard_sink(void *user, uint64_t row, char const *bytes, uint64_t length)
	{
		auto const &st(*static_cast<shard_state *>(user));
		std::uint64_t const i(st.first + row);
		std::string const header(">" + (*st.ids)[i] + "\n");
		char newline('\n');
		// header, body, newline as one gather list, written in turns of at most kTurnBytes: the contexts' threads alternate at that grain,
		// so that on a file system whose writes to one file do run in parallel (not tmpfs / ext4 under buffered I/O, where the inode lock
		// serialises them anyway: profiles/r04/e2e_config2_file_destinations.txt) a 100-MB row does not hold the others up for its whole length
		constexpr std::size_t kTurnBytes(std::size_t(16) << 20);
		struct iovec iov[3] = {{const_cast<char *>(header.data()), header.size()}, {const_cast<char *>(bytes), length}, {&newline, 1}};
		std::uint64_t off(st.offsets[i]);
		int k(0);
		while (k < 3) {   // pwritev may write less than asked
			struct iovec turn[3];
			int n(0);
			std::size_t budget(kTurnBytes);
			for (int j(k); j < 3 && budget; ++j) {
				turn[n] = iov[j];
				if (turn[n].iov_len > budget) turn[n].iov_len = budget;
				budget -= turn[n].iov_len;
				++n;
			}
			ssize_t w;
			{
				std::lock_guard<std::mutex> const lock(*st.one_writer);
				w = ::pwritev(st.fd, turn, n, off_t(off));
			}
			if (w < 0 && EINTR == errno) continue;
			if (w <= 0) return 1;
			off += std::uint64_t(w);
			std::size_t left = std::size_t(w);
			while (k < 3 && left >= iov[k].iov_len) { left -= iov[k].iov_len; ++k; }
			if (k < 3) { iov[k].iov_base = static_cast<char *>(iov[k].iov_base) + left; iov[k].iov_len -= left; }
		}
		return 0;
	}
}


void output::write_a2m_sharded(row_set const &rows, char const *dst_name)
{
	std::vector<gpu_context *> gpus{&m_gpu};
	gpus.insert(gpus.end(), m_more_gpus.begin(), m_more_gpus.end());
	std::uint64_t const n(rows.copy_index.size()), L(v2m_window_length(m_gpu.get()));   // the column window's length when one is set (every context has the same)
	std::vector<std::uint64_t> offsets(n + 1, 0);
	for (std::uint64_t i(0); i < n; ++i) offsets[i + 1] = offsets[i] + 1 + rows.ids[i].size() + 1 + L + 1;   // '>' id '\n' body '\n'

	int const fd(::open(dst_name, O_WRONLY | O_CREAT | O_TRUNC, 0644));
	if (fd < 0) throw std::runtime_error(std::string("unable to open ") + dst_name + " for writing");
	struct closer { int fd; ~closer() { ::close(fd); } } const close_on_exit{fd};
	if (0 != ::ftruncate(fd, off_t(offsets[n]))) { /* not all targets can be sized (e.g. /dev/null); pwrite extends regular files anyway */ }

	std::size_t const g(gpus.size());
	// Which rows go to which context: with a sharded path matrix, the rows whose copy the context holds (REF: the first
	// context); otherwise equal contiguous blocks.  Rows are in copy order (haplotype_output.cc:62-65), so either way a
	// context's rows are one contiguous block of the file.
	std::vector<std::uint64_t> bounds(g + 1, n);
	bounds[0] = 0;
	bool const sharded(!m_copy_shards.empty());
	if (sharded) {
		if (m_copy_shards.size() != g) throw std::runtime_error("one copy shard per GPU context is needed");
		if (rows.any_cuts) throw std::runtime_error("rows that switch copies need the whole path matrix on every GPU");
		std::uint64_t i(0);
		for (std::size_t k(0); k < g; ++k) {
			while (i < n && (V2M_PLOIDY_MAX == rows.copy_index[i] ? 0 == k : rows.copy_index[i] < m_copy_shards[k].end)) ++i;
			bounds[k + 1] = i;
		}
		if (bounds[g] != n) throw std::runtime_error("a row's chromosome copy lies outside every GPU's shard");
	} else {
		for (std::size_t k(0); k <= g; ++k) bounds[k] = n * k / g;
	}
	std::vector<std::exception_ptr> errors(g);
	std::mutex one_writer;
	std::vector<std::thread> threads;
	for (std::size_t k(0); k < g; ++k) {
		std::uint64_t const first(bounds[k]), last(bounds[k + 1]);
		threads.emplace_back([&, k, first, last] {
			try {
				if (first == last) return;
				v2m_row_batch batch{};
				batch.n_rows = last - first;
				batch.copy_index = rows.copy_index.data() + first;
				std::vector<std::uint32_t> rebased;
				if (sharded) {
					rebased = rebased_copies(rows, first, last, m_copy_shards[k]);
					batch.copy_index = rebased.data();
				}
				std::vector<std::uint64_t> cut_offsets;
				if (rows.any_cuts) {   // re-base the CSR offsets of the shard
					cut_offsets.assign(rows.cut_offsets.begin() + first, rows.cut_offsets.begin() + last + 1);
					std::uint64_t const base(cut_offsets.front());
					for (auto &o : cut_offsets) o -= base;
					batch.cut_offsets = cut_offsets.data();
					batch.cut_nodes = rows.cut_nodes.data() + base;
					batch.cut_copies = rows.cut_copies.data() + base;
				}
				shard_state st{fd, &rows.ids, offsets.data(), first, &one_writer};
				gpus[k]->check(v2m_splice_rows(gpus[k]->get(), &batch, 0u, shard_sink, &st));
			} catch (...) {
				errors[k] = std::current_exception();
			}
		});
	}
	for (auto &t : threads) t.join();
	for (auto const &e : errors) if (e) std::rethrow_exception(e);
	for (std::uint64_t i(0); i < n; ++i) m_delegate->handled_sequences(u32(1 + i));
}


void output::output_a2m(variant_graph const &graph, char const *dst_name)          // output.cc:47-76
{
	if (m_pipe_cmd) {                                                               // :49-68
		pipe_process proc(m_pipe_cmd, dst_name);
		bool good(false);
		std::exception_ptr error;
		try {
			fd_streambuf buf(proc.fd());
			std::ostream stream(&buf);
			output_a2m(graph, stream);
			stream.flush();
			good = stream.good();
		} catch (...) {
			error = std::current_exception();
		}
		proc.finish();                                                              // a failed child is the more telling error
		if (error) std::rethrow_exception(error);
		if (!good) throw std::runtime_error(std::string("error while writing to the subprocess for ") + dst_name);
		return;
	}
	if (!m_more_gpus.empty() && !m_should_output_unaligned && !m_interleaved && !m_bgzf) {
		write_a2m_sharded(a2m_rows(graph), dst_name);
		return;
	}
	std::ofstream stream(dst_name, std::ios::binary | std::ios::trunc);
	if (!stream) throw std::runtime_error(std::string("unable to open ") + dst_name + " for writing");
	output_a2m(graph, stream);
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + dst_name);
}


// --- chains (--output-chain) ----------------------------------------------------------------------------------
std::string chain_text(v2m_aln_op const *ops, u64 n_ops, std::string const &t_name, u64 t_size, std::string const &q_name, u64 q_size, u64 id)
{
	u64 first(n_ops), last(0), score(0);
	for (u64 i(0); i < n_ops; ++i) {
		if (ops[i].op > V2M_OP_D) throw std::invalid_argument("alignment op code " + std::to_string(ops[i].op) + " is none of M, I, D");
		if (V2M_OP_M != ops[i].op) continue;
		if (n_ops == first) first = i;
		last = i;
		score += ops[i].length;
	}
	if (n_ops == first) return std::string();
	u64 t_start(0), q_start(0), t_end(t_size), q_end(q_size);
	for (u64 i(0); i < first; ++i) (V2M_OP_D == ops[i].op ? t_start : q_start) += ops[i].length;
	for (u64 i(last + 1); i < n_ops; ++i) (V2M_OP_D == ops[i].op ? t_end : q_end) -= ops[i].length;
	std::string text("chain " + std::to_string(score) + ' ' + t_name + ' ' + std::to_string(t_size) + " + " + std::to_string(t_start) + ' ' + std::to_string(t_end)
		+ ' ' + q_name + ' ' + std::to_string(q_size) + " + " + std::to_string(q_start) + ' ' + std::to_string(q_end) + ' ' + std::to_string(id) + '\n');
	u64 size(ops[first].length), dt(0), dq(0);
	for (u64 i(first + 1); i <= last; ++i) {
		if (V2M_OP_D == ops[i].op) dt += ops[i].length;
		else if (V2M_OP_I == ops[i].op) dq += ops[i].length;
		else if (0 == dt && 0 == dq) size += ops[i].length;   // (two M ops in a row: one block)
		else {
			text += std::to_string(size) + ' ' + std::to_string(dt) + ' ' + std::to_string(dq) + '\n';
			size = ops[i].length;
			dt = dq = 0;
		}
	}
	text += std::to_string(size) + "\n\n";
	return text;
}


// --- PAF (--output-paf) -----------------------------------------------------------------------------------------
std::string paf_text(v2m_aln_op const *ops, u64 n_ops, std::string const &t_name, u64 t_size, std::string const &q_name, u64 q_size)
{
	auto const aligned([](v2m_aln_op const &op) { return V2M_OP_EQ == op.op || V2M_OP_X == op.op; });
	u64 first(n_ops), last(0);
	for (u64 i(0); i < n_ops; ++i) {
		if (!aligned(ops[i]) && V2M_OP_I != ops[i].op && V2M_OP_D != ops[i].op)
			throw std::invalid_argument("alignment op code " + std::to_string(ops[i].op) + " is none of =, X, I, D (ops made with V2M_OPS_SPLIT_MATCH)");
		if (!aligned(ops[i])) continue;
		if (n_ops == first) first = i;
		last = i;
	}
	if (n_ops == first) return std::string();
	u64 t_start(0), q_start(0), t_end(t_size), q_end(q_size);
	for (u64 i(0); i < first; ++i) (V2M_OP_D == ops[i].op ? t_start : q_start) += ops[i].length;
	for (u64 i(last + 1); i < n_ops; ++i) (V2M_OP_D == ops[i].op ? t_end : q_end) -= ops[i].length;
	u64 n_eq(0), block_len(0);
	std::string cigar;
	for (u64 i(first); i <= last; ++i) {
		block_len += ops[i].length;
		if (V2M_OP_EQ == ops[i].op) n_eq += ops[i].length;
		cigar += std::to_string(ops[i].length);
		cigar += V2M_OP_EQ == ops[i].op ? '=' : V2M_OP_X == ops[i].op ? 'X' : V2M_OP_I == ops[i].op ? 'I' : 'D';
	}
	return q_name + '\t' + std::to_string(q_size) + '\t' + std::to_string(q_start) + '\t' + std::to_string(q_end) + "\t+\t"
		+ t_name + '\t' + std::to_string(t_size) + '\t' + std::to_string(t_start) + '\t' + std::to_string(t_end) + '\t'
		+ std::to_string(n_eq) + '\t' + std::to_string(block_len) + "\t255\tNM:i:" + std::to_string(block_len - n_eq) + "\tcg:Z:" + cigar + '\n';
}


std::vector<v2m_aln_op> fold_split_ops(v2m_aln_op const *ops, u64 n_ops)
{
	std::vector<v2m_aln_op> folded;
	folded.reserve(n_ops);
	for (u64 i(0); i < n_ops; ++i) {
		u32 const op(V2M_OP_EQ == ops[i].op || V2M_OP_X == ops[i].op ? V2M_OP_M : ops[i].op);
		if (!folded.empty() && folded.back().op == op) folded.back().length += ops[i].length;
		else folded.push_back(v2m_aln_op{op, ops[i].length});
	}
	return folded;
}


namespace {
	// chain and paf: either may be null; with paf the ops are split ones, and the chain is made from them folded back
	struct chain_state { std::ostream *chain, *paf; std::vector<std::string> const *names; std::string const *t_name; std::exception_ptr error; };

	int chain_sink(void *user, uint64_t row, v2m_aln_op const *ops, uint64_t n_ops, uint64_t row_length)
	{
		auto &st(*static_cast<chain_state *>(user));
		try {
			u64 t_size(0);
			for (u64 i(0); i < n_ops; ++i) if (V2M_OP_I != ops[i].op) t_size += ops[i].length;
			if (st.chain) {
				std::vector<v2m_aln_op> folded;
				if (st.paf) folded = fold_split_ops(ops, n_ops);
				std::string const text(st.paf ? chain_text(folded.data(), folded.size(), *st.t_name, t_size, (*st.names)[row], row_length, row + 1)
					: chain_text(ops, n_ops, *st.t_name, t_size, (*st.names)[row], row_length, row + 1));
				if (text.empty()) std::fprintf(stderr, "Warning: %s shares no column with the reference; it gets no chain.\n", (*st.names)[row].c_str());
				else st.chain->write(text.data(), std::streamsize(text.size()));
				if (!st.chain->good()) return 1;
			}
			if (st.paf) {
				std::string const text(paf_text(ops, n_ops, *st.t_name, t_size, (*st.names)[row], row_length));
				if (text.empty()) std::fprintf(stderr, "Warning: %s shares no column with the reference; it gets no PAF line.\n", (*st.names)[row].c_str());
				else st.paf->write(text.data(), std::streamsize(text.size()));
				if (!st.paf->good()) return 1;
			}
			return 0;
		} catch (...) {   // nothing may cross the C boundary
			st.error = std::current_exception();
			return 1;
		}
	}
}


void output::output_chain(variant_graph const &graph, std::ostream &stream)
{
	write_chains(graph, [&stream]() -> std::ostream & { return stream; });
}


void output::write_chains(variant_graph const &graph, std::function<std::ostream &()> const &open_chain, std::function<std::ostream &()> const &open_paf)
{
	char const *const what(open_chain ? "--output-chain" : "--output-paf");
	if (!m_more_gpus.empty()) throw std::runtime_error(std::string(what) + " needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error(std::string(what) + " needs every chromosome copy on one GPU context");
	row_set const all(chain_rows(graph));
	std::string const t_name(prefixed("REF", '.'));
	auto const has_space([](std::string const &s) { return std::any_of(s.begin(), s.end(), [](char c) { return std::isspace(static_cast<unsigned char>(c)); }); });
	if (has_space(t_name)) throw std::runtime_error("the chain's target name \"" + t_name + "\" holds whitespace");
	// the rows but REF (the row that follows no copy and has no cuts)
	row_set rows;
	rows.any_cuts = all.any_cuts;
	for (std::size_t r(0); r < all.copy_index.size(); ++r) {
		bool const has_cuts(all.any_cuts && all.cut_offsets[r + 1] != all.cut_offsets[r]);
		if (V2M_PLOIDY_MAX == all.copy_index[r] && !has_cuts) continue;
		if (has_space(all.ids[r])) throw std::runtime_error("the sequence name \"" + all.ids[r] + "\" holds whitespace, which a chain's qName cannot");
		rows.ids.push_back(all.ids[r]);
		rows.copy_index.push_back(all.copy_index[r]);
		if (all.any_cuts) {
			rows.cut_nodes.insert(rows.cut_nodes.end(), all.cut_nodes.begin() + all.cut_offsets[r], all.cut_nodes.begin() + all.cut_offsets[r + 1]);
			rows.cut_copies.insert(rows.cut_copies.end(), all.cut_copies.begin() + all.cut_offsets[r], all.cut_copies.begin() + all.cut_offsets[r + 1]);
			rows.cut_offsets.push_back(rows.cut_nodes.size());
		}
	}
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	chain_state st{open_chain ? &open_chain() : nullptr, open_paf ? &open_paf() : nullptr, &rows.ids, &t_name, nullptr};
	int const rc(v2m_row_ops(m_gpu.get(), &batch, open_paf ? V2M_OPS_SPLIT_MATCH : 0, chain_sink, &st));
	if (st.error) std::rethrow_exception(st.error);
	m_gpu.check(rc);
}


void output::output_chain(variant_graph const &graph, char const *path)
{
	std::ofstream stream;
	write_chains(graph, [&]() -> std::ostream & {
		stream.open(path, std::ios::binary | std::ios::trunc);
		if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
		return stream;
	});
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
}


void output::output_paf(variant_graph const &graph, std::ostream &stream)
{
	write_chains(graph, {}, [&stream]() -> std::ostream & { return stream; });
}


void output::output_chain_and_paf(variant_graph const &graph, std::ostream &chain_stream, std::ostream &paf_stream)
{
	write_chains(graph, [&chain_stream]() -> std::ostream & { return chain_stream; }, [&paf_stream]() -> std::ostream & { return paf_stream; });
}


namespace {
	std::function<std::ostream &()> opener(std::ofstream &stream, char const *path)
	{
		return [&stream, path]() -> std::ostream & {
			stream.open(path, std::ios::binary | std::ios::trunc);
			if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
			return stream;
		};
	}

	void finish(std::ofstream &stream, char const *path)
	{
		stream.flush();
		if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
	}
}


void output::output_paf(variant_graph const &graph, char const *path)
{
	std::ofstream stream;
	write_chains(graph, {}, opener(stream, path));
	finish(stream, path);
}


void output::output_chain_and_paf(variant_graph const &graph, char const *chain_path, char const *paf_path)
{
	std::ofstream chain_stream, paf_stream;
	write_chains(graph, opener(chain_stream, chain_path), opener(paf_stream, paf_path));
	finish(chain_stream, chain_path);
	finish(paf_stream, paf_path);
}


// --- column counts (--output-column-counts) ---------------------------------------------------------------------
namespace {
	// One line per record, appended to `text`.  `node` carries the graph position from one record to the next (records ascend; a
	// record that does not is looked up afresh).
	// The first two fields of a line: the column and the reference position the REF row holds there ('.' where it holds padding).
	void append_column_and_position(std::string &text, u64 column, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count, u64 &node)
	{
		// the last node n with aligned_positions[n] <= column
		if (node >= node_count || aligned_positions[node] > column)
		{
			u64 const above(u64(std::upper_bound(aligned_positions, aligned_positions + node_count, column) - aligned_positions));
			node = above ? above - 1 : 0;
		}
		while (node + 1 < node_count && aligned_positions[node + 1] <= column) ++node;
		text += std::to_string(column);
		text += '\t';
		bool has_ref(false);
		if (node + 1 < node_count && aligned_positions[node] <= column) {
			u64 const k(column - aligned_positions[node]);
			if (k < reference_positions[node + 1] - reference_positions[node]) {
				text += std::to_string(reference_positions[node] + k + 1);
				has_ref = true;
			}
		}
		if (!has_ref) text += '.';   // the REF row has padding there
	}

	void append_column_count_lines(std::string &text, u64 n_rows, v2m_column_count const *records, u64 n_records,
		u64 const *reference_positions, u64 const *aligned_positions, u64 node_count, u64 &node)
	{
		for (u64 i(0); i < n_records; ++i) {
			v2m_column_count const &rec(records[i]);
			append_column_and_position(text, rec.column, reference_positions, aligned_positions, node_count, node);
			u64 sum(0);
			for (u32 const c : rec.count) {
				text += '\t';
				text += std::to_string(c);
				sum += c;
			}
			text += '\t';
			text += std::to_string(n_rows - sum);
			text += '\n';
		}
	}

	std::string column_counts_header(u64 n_rows)
	{
		return "#rows\t" + std::to_string(n_rows) + "\n#column\tref_pos\tA\tC\tG\tT\tN\tgap\tother\n";
	}

	struct column_counts_state {
		std::ostream *stream;
		u64 n_rows, n_records, n_variable, node;
		variant_graph const *graph;
		std::string text;
		std::exception_ptr error;
	};

	int column_counts_sink(void *user, v2m_column_count const *records, uint64_t n)
	{
		auto &st(*static_cast<column_counts_state *>(user));
		try {
			st.text.clear();
			append_column_count_lines(st.text, st.n_rows, records, n, st.graph->reference_positions.data(), st.graph->aligned_positions.data(), st.graph->node_count(), st.node);
			st.stream->write(st.text.data(), std::streamsize(st.text.size()));
			st.n_records += n;
			for (u64 i(0); i < n; ++i) {   // (variable: none of the seven classes holds every row)
				u64 sum(0), most(0);
				for (u32 const c : records[i].count) { sum += c; most = std::max<u64>(most, c); }
				if (std::max(most, st.n_rows - sum) != st.n_rows) ++st.n_variable;
			}
			return st.stream->good() ? 0 : 1;
		} catch (...) {   // nothing may cross the C boundary
			st.error = std::current_exception();
			return 1;
		}
	}
}


std::string column_counts_text(u64 n_rows, v2m_column_count const *records, u64 n_records, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count)
{
	std::string text(column_counts_header(n_rows));
	u64 node(0);
	append_column_count_lines(text, n_rows, records, n_records, reference_positions, aligned_positions, node_count, node);
	return text;
}


void output::output_column_counts(variant_graph const &graph, std::ostream &stream, bool all_columns, bool verbose)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-column-counts needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-column-counts needs every chromosome copy on one GPU context");
	row_set const rows(a2m_rows(graph));
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	std::string const header(column_counts_header(batch.n_rows));
	stream.write(header.data(), std::streamsize(header.size()));
	column_counts_state st{&stream, batch.n_rows, 0, 0, 0, &graph, {}, nullptr};
	int const rc(v2m_column_counts(m_gpu.get(), &batch, all_columns ? 0 : V2M_COUNTS_VARIABLE_ONLY, column_counts_sink, &st));
	if (st.error) std::rethrow_exception(st.error);
	m_gpu.check(rc);
	if (verbose)
		std::fprintf(stderr, "Column counts: %llu rows, %llu columns, %llu variable.\n", (unsigned long long) batch.n_rows, (unsigned long long) v2m_window_length(m_gpu.get()),
			(unsigned long long) st.n_variable);
}


void output::output_column_counts(variant_graph const &graph, char const *path, bool all_columns, bool verbose)
{
	std::ofstream stream(path, std::ios::binary | std::ios::trunc);
	if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
	output_column_counts(graph, stream, all_columns, verbose);
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
}


// --- pair distances (--output-distances) ------------------------------------------------------------------------
std::string distances_text(std::vector<std::string> const &ids, std::uint32_t const *dist, u64 n_columns, u64 n_sites, bool acgt_only)
{
	u64 const n(ids.size());
	for (auto const &id : ids)
		if (std::string::npos != id.find_first_of("\t\n\r")) throw std::runtime_error("the sequence name \"" + id + "\" holds a tab or a line break, which a cell of the distance table cannot");
	std::string text("#rows\t" + std::to_string(n) + "\tcolumns\t" + std::to_string(n_columns) + "\tsites\t" + std::to_string(n_sites) + "\tmodel\t" + (acgt_only ? "acgt" : "all") + "\nid");
	for (auto const &id : ids) { text += '\t'; text += id; }
	text += '\n';
	for (u64 i(0); i < n; ++i) {
		text += ids[i];
		for (u64 j(0); j < n; ++j) { text += '\t'; text += std::to_string(dist[i * n + j]); }
		text += '\n';
	}
	return text;
}


void output::output_distances(variant_graph const &graph, std::ostream &stream, bool acgt_only, bool verbose)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-distances needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-distances needs every chromosome copy on one GPU context");
	row_set const rows(chain_rows(graph));   // (the rows of a2m_rows() under the names --output-paf writes)
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	std::vector<std::uint32_t> dist(std::max<std::size_t>(1, std::size_t(batch.n_rows) * batch.n_rows));
	v2m_pair_distances_info info{};
	info.n_columns = v2m_window_length(m_gpu.get());
	m_gpu.check(v2m_pair_distances(m_gpu.get(), &batch, acgt_only ? V2M_DIST_ACGT_ONLY : 0, dist.data(), &info));
	std::string const text(distances_text(rows.ids, dist.data(), info.n_columns, info.n_sites, acgt_only));
	stream.write(text.data(), std::streamsize(text.size()));
	if (verbose)
		std::fprintf(stderr, "Distances: %llu rows, %llu columns, %llu sites, %llu passes.\n", (unsigned long long) batch.n_rows, (unsigned long long) info.n_columns,
			(unsigned long long) info.n_sites, (unsigned long long) info.n_passes);
}


void output::output_distances(variant_graph const &graph, char const *path, bool acgt_only, bool verbose)
{
	std::ofstream stream(path, std::ios::binary | std::ios::trunc);
	if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
	output_distances(graph, stream, acgt_only, verbose);
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
}


// --- variable sites (--output-variable-sites) ---------------------------------------------------------------------
std::string site_positions_text(u64 const *columns, u64 n_sites, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count)
{
	std::string text;
	u64 node(0);
	for (u64 i(0); i < n_sites; ++i) {
		append_column_and_position(text, columns[i], reference_positions, aligned_positions, node_count, node);
		text += '\n';
	}
	return text;
}


namespace {
	struct variable_sites_state {
		std::ostream *stream;
		std::ostream *positions;
		std::vector<std::string> const *ids;
		variant_graph const *graph;
		u64 next_row;
		std::exception_ptr error;
	};

	int variable_sites_columns_sink(void *user, uint64_t const *columns, uint64_t n_sites)
	{
		auto &st(*static_cast<variable_sites_state *>(user));
		if (!st.positions) return 0;
		try {
			std::string const text(site_positions_text(columns, n_sites, st.graph->reference_positions.data(), st.graph->aligned_positions.data(), st.graph->node_count()));
			st.positions->write(text.data(), std::streamsize(text.size()));
			return st.positions->good() ? 0 : 1;
		} catch (...) {   // nothing may cross the C boundary
			st.error = std::current_exception();
			return 1;
		}
	}

	int variable_sites_rows_sink(void *user, uint64_t first_row, uint64_t n_rows, char const *bytes, uint64_t pitch, uint64_t n_sites)
	{
		auto &st(*static_cast<variable_sites_state *>(user));
		try {
			if (first_row != st.next_row) throw std::runtime_error("the rows of the variable sites arrived out of order");
			for (u64 r(0); r < n_rows; ++r) {
				*st.stream << '>' << (*st.ids)[first_row + r] << '\n';   // as a2m_sink writes a row
				st.stream->write(bytes + r * pitch, std::streamsize(n_sites));
				*st.stream << '\n';
			}
			st.next_row = first_row + n_rows;
			return st.stream->good() ? 0 : 1;
		} catch (...) {
			st.error = std::current_exception();
			return 1;
		}
	}
}


void output::output_variable_sites(variant_graph const &graph, std::ostream &stream, bool snp_only, std::ostream *positions, bool verbose)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-variable-sites needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-variable-sites needs every chromosome copy on one GPU context");
	row_set const rows(a2m_rows(graph));   // (the rows and the names of the -s file)
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	variable_sites_state st{&stream, positions, &rows.ids, &graph, 0, nullptr};
	v2m_variable_sites_info info{};
	info.n_columns = v2m_window_length(m_gpu.get());
	int const rc(v2m_variable_sites(m_gpu.get(), &batch, snp_only ? V2M_SITES_SNP : 0, variable_sites_columns_sink, variable_sites_rows_sink, &st, &info));
	if (st.error) std::rethrow_exception(st.error);
	m_gpu.check(rc);
	if (0 == info.n_sites)   // no site, no delivery: every sequence line is empty
		for (auto const &id : rows.ids) stream << '>' << id << "\n\n";
	if (verbose)
		std::fprintf(stderr, "Variable sites: %llu rows, %llu columns, %llu sites.\n", (unsigned long long) batch.n_rows, (unsigned long long) info.n_columns,
			(unsigned long long) info.n_sites);
}


void output::output_variable_sites(variant_graph const &graph, char const *path, bool snp_only, char const *positions_path, bool verbose)
{
	std::ofstream stream(path, std::ios::binary | std::ios::trunc);
	if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
	std::ofstream positions;
	if (positions_path) {
		positions.open(positions_path, std::ios::binary | std::ios::trunc);
		if (!positions) throw std::runtime_error(std::string("unable to open ") + positions_path + " for writing");
	}
	output_variable_sites(graph, stream, snp_only, positions_path ? &positions : nullptr, verbose);
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
	if (positions_path) {
		positions.flush();
		if (!positions) throw std::runtime_error(std::string("error while writing ") + positions_path);
	}
}


// --- site LD (--output-ld) ----------------------------------------------------------------------------------------
bool parse_decimal_fraction(char const *text, std::uint32_t &numerator, std::uint32_t &denominator)
{
	std::string const s(text);
	auto const dot(s.find('.'));
	std::string const whole(s.substr(0, dot)), decimals(std::string::npos == dot ? std::string() : s.substr(dot + 1));
	if (whole.empty() || whole.size() > 7 || decimals.size() > 6) return false;
	if (std::string::npos != whole.find_first_not_of("0123456789") || std::string::npos != decimals.find_first_not_of("0123456789")) return false;
	u64 den(1);
	for (std::size_t i(0); i < decimals.size(); ++i) den *= 10;
	u64 num(std::stoull(whole) * den + (decimals.empty() ? 0 : std::stoull(decimals)));
	if (num > den) return false;
	u64 a(num), b(den);
	while (b) { u64 const r(a % b); a = b; b = r; }   // (a = gcd >= 1: den >= 1)
	numerator = std::uint32_t(num / a);
	denominator = std::uint32_t(den / a);
	return true;
}


std::string site_ld_text(u64 n_rows, u64 n_columns, v2m_ld_site const *sites, u64 n_sites, v2m_ld_pair const *pairs, u64 n_pairs, v2m_site_ld_params const &params,
	u64 const *reference_positions, u64 const *aligned_positions, u64 node_count)
{
	std::string text("#rows\t" + std::to_string(n_rows) + "\tcolumns\t" + std::to_string(n_columns) + "\tsites\t" + std::to_string(n_sites) + "\tpairs\t" + std::to_string(n_pairs)
		+ "\twindow\t" + std::to_string(params.window_sites) + "\twindow_columns\t" + std::to_string(params.window_columns)
		+ "\tmin_r2\t" + std::to_string(params.min_r2_num) + "/" + std::to_string(params.min_r2_den) + "\tmin_count\t" + std::to_string(params.min_allele_count)
		+ "\n#column_a\tpos_a\tcolumn_b\tpos_b\tn\tn_a\tn_b\tn_ab\tr2\n");
	u64 node_a(0), node_b(0);
	char r2[64];
	for (u64 i(0); i < n_pairs; ++i) {
		v2m_ld_pair const &p(pairs[i]);
		if (p.site_a >= n_sites || p.site_b >= n_sites) throw std::runtime_error("a pair of the site LD names a site beyond the last");
		std::int64_t const d(std::int64_t(u64(p.n) * p.n_ab) - std::int64_t(u64(p.n_a) * p.n_b));
		u64 const d2(u64(d * d)), den(u64(p.n_a) * (p.n - p.n_a) * (u64(p.n_b) * (p.n - p.n_b)));
		if (0 == den) throw std::runtime_error("a pair of the site LD has a denominator of 0");
		append_column_and_position(text, sites[p.site_a].column, reference_positions, aligned_positions, node_count, node_a);
		text += '\t';
		append_column_and_position(text, sites[p.site_b].column, reference_positions, aligned_positions, node_count, node_b);
		for (u32 const c : {p.n, p.n_a, p.n_b, p.n_ab}) { text += '\t'; text += std::to_string(c); }
		std::snprintf(r2, sizeof(r2), "\t%.6f\n", double(d2) / double(den));
		text += r2;
	}
	return text;
}


namespace {
	struct site_ld_state {
		std::vector<v2m_ld_site> sites;
		std::vector<v2m_ld_pair> pairs;
		std::exception_ptr error;
	};

	int site_ld_sites_sink(void *user, v2m_ld_site const *sites, uint64_t n)
	{
		auto &st(*static_cast<site_ld_state *>(user));
		try {
			st.sites.assign(sites, sites + n);
			return 0;
		} catch (...) {   // nothing may cross the C boundary
			st.error = std::current_exception();
			return 1;
		}
	}

	int site_ld_pairs_sink(void *user, v2m_ld_pair const *pairs, uint64_t n)
	{
		auto &st(*static_cast<site_ld_state *>(user));
		try {
			st.pairs.insert(st.pairs.end(), pairs, pairs + n);
			return 0;
		} catch (...) {
			st.error = std::current_exception();
			return 1;
		}
	}
}


void output::output_ld(variant_graph const &graph, std::ostream &stream, v2m_site_ld_params const &params, bool verbose)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-ld needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-ld needs every chromosome copy on one GPU context");
	row_set const rows(a2m_rows(graph));
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	site_ld_state st;
	v2m_site_ld_info info{};
	info.n_columns = v2m_window_length(m_gpu.get());
	int const rc(v2m_site_ld(m_gpu.get(), &batch, &params, site_ld_sites_sink, site_ld_pairs_sink, &st, &info));
	if (st.error) std::rethrow_exception(st.error);
	m_gpu.check(rc);
	std::string const text(site_ld_text(batch.n_rows, info.n_columns, st.sites.data(), st.sites.size(), st.pairs.data(), st.pairs.size(), params,
		graph.reference_positions.data(), graph.aligned_positions.data(), graph.node_count()));
	stream.write(text.data(), std::streamsize(text.size()));
	if (verbose)
		std::fprintf(stderr, "Site LD: %llu rows, %llu columns, %llu sites, %llu candidates, %llu pairs.\n", (unsigned long long) batch.n_rows, (unsigned long long) info.n_columns,
			(unsigned long long) info.n_sites, (unsigned long long) info.n_candidates, (unsigned long long) info.n_pairs);
}


void output::output_ld(variant_graph const &graph, char const *path, v2m_site_ld_params const &params, bool verbose)
{
	std::ofstream stream(path, std::ios::binary | std::ios::trunc);
	if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
	output_ld(graph, stream, params, verbose);
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
}


// --- neighbour joining (--output-tree) ---------------------------------------------------------------------------
// The header's definition in plain loops.  Every operation of the definition is a statement of its own, and nothing here may be
// contracted: the host library is built as ISO C++ (-std=c++20, which sets -ffp-contract=off in g++) and without -march, so that the
// compiler neither fuses a product into a sum nor has an instruction to fuse them with.  The live taxa keep their places in `at`;
// the new node takes the place of a, and the place of b is dropped from the list of the live ones, which stays in ascending order of
// place -- the order plays no part: the pair is chosen by (Q, lower id, higher id).
void nj_tree_cpu(std::uint32_t const *dist, u64 n, u64 pitch, v2m_nj_node *nodes)
{
	if (n < 3) throw std::invalid_argument("a neighbour-joining tree needs at least 3 taxa");
	if (pitch < n) throw std::invalid_argument("the pitch of the distance matrix is smaller than its side");
	std::vector<double> D(n * n, 0.0), R(n, 0.0);
	std::vector<std::uint32_t> id(n), live(n);
	for (u64 i(0); i < n; ++i) {
		id[i] = std::uint32_t(i);
		live[i] = std::uint32_t(i);
		for (u64 j(i + 1); j < n; ++j) {
			double const d(double(dist[i * pitch + j]));
			D[i * n + j] = d;
			D[j * n + i] = d;
		}
	}
	for (u64 i(0); i < n; ++i) {
		double sum(0.0);   // (exact integers below 2^53: any order)
		for (u64 j(0); j < n; ++j) sum += D[i * n + j];
		R[i] = sum;
	}
	u64 t(0);
	for (u64 r(n); r > 3; --r, ++t) {
		double const factor = double(r - 2);
		bool have(false);
		double best_q(0.0);
		std::uint32_t best_lo(0), best_hi(0);
		u64 best_x(0), best_y(0);
		for (u64 x(0); x < r; ++x) {
			u64 const i(live[x]);
			double const *const row(&D[i * n]);
			for (u64 y(x + 1); y < r; ++y) {
				u64 const j(live[y]);
				double const product = factor * row[j];
				double const sum = R[i] + R[j];
				double const q = product - sum;
				if (have && q > best_q) continue;
				std::uint32_t const lo(std::min(id[i], id[j])), hi(std::max(id[i], id[j]));
				if (!have || q < best_q || lo < best_lo || (lo == best_lo && hi < best_hi)) {
					have = true; best_q = q; best_lo = lo; best_hi = hi; best_x = x; best_y = y;
				}
			}
		}
		bool const a_first(id[live[best_x]] == best_lo);
		u64 const pa(live[a_first ? best_x : best_y]), pb(live[a_first ? best_y : best_x]);
		double const d_ab = D[pa * n + pb];
		double const difference = R[pa] - R[pb];
		double const delta = difference / factor;
		double const with_delta = d_ab + delta;
		double const len_a = 0.5 * with_delta;
		double const len_b = d_ab - len_a;
		nodes[t] = v2m_nj_node{best_lo, best_hi, V2M_NJ_NONE, 0, len_a, len_b, 0.0};
		double const both = R[pa] + R[pb];
		double const product = double(r) * d_ab;
		double const remainder = both - product;
		double const r_u = 0.5 * remainder;
		for (u64 x(0); x < r; ++x) {
			u64 const k(live[x]);
			if (k == pa || k == pb) continue;
			double const s = D[pa * n + k] + D[pb * n + k];
			double const less = s - d_ab;
			double const d_uk = 0.5 * less;
			double const without = R[k] - s;
			R[k] = without + d_uk;
			D[pa * n + k] = d_uk;
			D[k * n + pa] = d_uk;
		}
		R[pa] = r_u;
		id[pa] = std::uint32_t(n + t);
		live.erase(live.begin() + std::ptrdiff_t(a_first ? best_y : best_x));
	}
	u64 p[3] = {live[0], live[1], live[2]};
	std::sort(p, p + 3, [&](u64 x, u64 y) { return id[x] < id[y]; });
	double const d_ab = D[p[0] * n + p[1]], d_ac = D[p[0] * n + p[2]], d_bc = D[p[1] * n + p[2]];
	double const ab_ac = d_ab + d_ac, ab_bc = d_ab + d_bc, ac_bc = d_ac + d_bc;
	double const for_a = ab_ac - d_bc, for_b = ab_bc - d_ac, for_c = ac_bc - d_ab;
	nodes[t] = v2m_nj_node{id[p[0]], id[p[1]], id[p[2]], 0, 0.5 * for_a, 0.5 * for_b, 0.5 * for_c};
}


namespace {
std::string newick_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels, std::uint32_t const *support, std::uint32_t const *branch_changes = nullptr);
}

std::string nj_newick_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels)
{
	return newick_text(nodes, n_leaves, labels, nullptr);
}

std::string nj_newick_support_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels, std::uint32_t const *support)
{
	if (!support && n_leaves > 3) throw std::invalid_argument("support is NULL");
	static std::uint32_t const none(0);
	return newick_text(nodes, n_leaves, labels, support ? support : &none);
}

void nj_split_support(u64 n_leaves, v2m_nj_node const *main_nodes, v2m_nj_node const *replicate_nodes, u64 n_replicates, std::uint32_t *support)
{
	std::string const err(v2m::nj_split_support(n_leaves, main_nodes, replicate_nodes, n_replicates, support));
	if (!err.empty()) throw std::runtime_error(err);
}

namespace {
// support: NULL, or the labels of the join nodes; branch_changes: NULL, or the integer lengths by lower node, with every internal node labelled node<t>
std::string newick_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels, std::uint32_t const *support, std::uint32_t const *branch_changes)
{
	u64 const n(n_leaves);
	if (n < 3) throw std::invalid_argument("a tree has at least 3 leaves");
	if (labels.size() != n) throw std::invalid_argument("the tree has " + std::to_string(n) + " leaves and " + std::to_string(labels.size()) + " labels");
	u64 const root(n - 3);   // the last record's index
	// the records are a tree over the leaves: every id but the root's is a child exactly once, and a node is made before it is joined
	std::vector<char> used(2 * n - 3, 0);
	for (u64 rec(0); rec <= root; ++rec) {
		v2m_nj_node const &nd(nodes[rec]);
		if ((rec < root) != (V2M_NJ_NONE == nd.c)) throw std::runtime_error("record " + std::to_string(rec) + " of the tree has " + (rec < root ? "three children" : "two children, and is the last"));
		for (int k(0); k < (rec < root ? 2 : 3); ++k) {
			u64 const child(0 == k ? nd.a : 1 == k ? nd.b : nd.c);
			if (child >= n + rec) throw std::runtime_error("record " + std::to_string(rec) + " of the tree names node " + std::to_string(child) + ", which is not made before it");
			if (used[child]) throw std::runtime_error("node " + std::to_string(child) + " of the tree is joined twice");
			used[child] = 1;
		}
	}
	auto const append_label([](std::string &text, std::string const &label) {
		bool bare(!label.empty());
		for (unsigned char const c : label) bare = bare && (std::isalnum(c) || '.' == c || '-' == c) && c < 0x80;
		if (bare) { text += label; return; }
		text += '\'';
		for (char const c : label) { if ('\'' == c) text += '\''; text += c; }
		text += '\'';
	});
	auto const append_length([](std::string &text, double len) {
		char buf[48];
		std::snprintf(buf, sizeof(buf), ":%.10g", len);
		text += buf;
	});
	struct frame { u64 rec; int next; };
	std::vector<frame> stack{{root, 0}};
	std::string text("(");
	while (!stack.empty()) {
		frame const f(stack.back());
		v2m_nj_node const &nd(nodes[f.rec]);
		int const children(f.rec == root ? 3 : 2);
		if (f.next > 0) {   // (of the child just closed)
			if (branch_changes) text += ':' + std::to_string(branch_changes[1 == f.next ? nd.a : 2 == f.next ? nd.b : nd.c]);
			else append_length(text, 1 == f.next ? nd.len_a : 2 == f.next ? nd.len_b : nd.len_c);
		}
		if (f.next == children) {
			text += ')';
			if (support && f.rec != root) text += std::to_string(support[f.rec]);
			if (branch_changes) text += "node" + std::to_string(f.rec);
			stack.pop_back();
			continue;
		}
		if (f.next > 0) text += ',';
		u64 const child(0 == f.next ? nd.a : 1 == f.next ? nd.b : nd.c);
		++stack.back().next;
		if (child < n) append_label(text, labels[child]);
		else {
			stack.push_back({child - n, 0});
			text += '(';
		}
	}
	text += ";\n";
	return text;
}
} // namespace


void output::output_tree(variant_graph const &graph, std::ostream &stream, bool acgt_only, bool verbose, std::uint32_t bootstrap, std::uint64_t seed, std::ostream *replicates)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-tree needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-tree needs every chromosome copy on one GPU context");
	row_set const rows(chain_rows(graph));   // (the rows of a2m_rows() under the names --output-distances writes)
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	if (batch.n_rows < 3) throw std::runtime_error("--output-tree needs at least three sequences (got " + std::to_string(batch.n_rows) + ")");
	std::vector<v2m_nj_node> nodes(batch.n_rows - 2);
	if (0 == bootstrap) {
		v2m_nj_tree_info info{};
		m_gpu.check(v2m_nj_tree(m_gpu.get(), &batch, acgt_only ? V2M_DIST_ACGT_ONLY : 0, nodes.data(), &info));
		std::string const text(nj_newick_text(nodes.data(), batch.n_rows, rows.ids));
		stream.write(text.data(), std::streamsize(text.size()));
		m_tree_nodes = nodes;
		if (verbose)
			std::fprintf(stderr, "Tree: %llu rows, %llu columns, %llu sites, %llu joins.\n", (unsigned long long) batch.n_rows, (unsigned long long) info.n_columns,
				(unsigned long long) info.n_sites, (unsigned long long) (info.n_nodes - 1));
		return;
	}
	std::vector<std::uint32_t> support(batch.n_rows - 3);
	std::vector<v2m_nj_node> replicate_nodes(replicates ? std::size_t(bootstrap) * nodes.size() : 0);
	v2m_nj_bootstrap_info info{};
	m_gpu.check(v2m_nj_bootstrap(m_gpu.get(), &batch, acgt_only ? V2M_DIST_ACGT_ONLY : 0, bootstrap, seed, nodes.data(), support.data(),
		replicates ? replicate_nodes.data() : nullptr, &info));
	std::string const text(nj_newick_support_text(nodes.data(), batch.n_rows, rows.ids, support.data()));
	stream.write(text.data(), std::streamsize(text.size()));
	m_tree_nodes = nodes;
	if (replicates) {
		for (std::uint32_t r(0); r < bootstrap; ++r) {
			std::string const line(nj_newick_text(replicate_nodes.data() + std::size_t(r) * nodes.size(), batch.n_rows, rows.ids));
			replicates->write(line.data(), std::streamsize(line.size()));
		}
	}
	if (verbose)
		std::fprintf(stderr, "Tree: %llu rows, %llu columns, %llu sites, %llu joins; %llu replicates, K = %llu, %llu pack passes.\n", (unsigned long long) batch.n_rows,
			(unsigned long long) info.n_columns, (unsigned long long) info.n_sites, (unsigned long long) (batch.n_rows - 3), (unsigned long long) info.n_replicates,
			(unsigned long long) info.max_slices, (unsigned long long) info.n_pack_passes);
}


void output::output_tree(variant_graph const &graph, char const *path, bool acgt_only, bool verbose, std::uint32_t bootstrap, std::uint64_t seed, char const *replicates_path)
{
	std::ofstream stream(path, std::ios::binary | std::ios::trunc);
	if (!stream) throw std::runtime_error(std::string("unable to open ") + path + " for writing");
	std::ofstream replicates;
	if (replicates_path) {
		replicates.open(replicates_path, std::ios::binary | std::ios::trunc);
		if (!replicates) throw std::runtime_error(std::string("unable to open ") + replicates_path + " for writing");
	}
	output_tree(graph, stream, acgt_only, verbose, bootstrap, seed, replicates_path ? &replicates : nullptr);
	stream.flush();
	if (!stream) throw std::runtime_error(std::string("error while writing ") + path);
	if (replicates_path) {
		replicates.flush();
		if (!replicates) throw std::runtime_error(std::string("error while writing ") + replicates_path);
	}
}


// --- parsimony on the tree ------------------------------------------------------------------------------------

u64 tree_parsimony_cpu(unsigned char const *bytes, u64 n, u64 n_sites, u64 pitch, v2m_nj_node const *nodes, v2m_parsimony_site *sites, std::uint32_t *branch_changes,
	v2m_tree_mutation *mutations, u64 capacity)
{
	{
		std::string err(n > V2M_NJ_MAX_ROWS ? std::string("more than V2M_NJ_MAX_ROWS taxa") : v2m::nj_records_error(nodes, n));
		for (u64 t(0); err.empty() && t < n - 2; ++t) {
			if (nodes[t].a >= nodes[t].b || (t == n - 3 && nodes[t].b >= nodes[t].c))
				err = "record " + std::to_string(t) + " of the tree does not name its children in ascending order";
		}
		if (!err.empty()) throw std::invalid_argument(err);
	}
	if (pitch < n_sites) throw std::invalid_argument("the pitch is smaller than the sites");
	auto const leaf_set([](unsigned char byte) -> unsigned {
		switch (byte | 0x20) {
			case 'a': return 1;
			case 'c': return 2;
			case 'g': return 4;
			case 't': return 8;
			default: return 0xF;
		}
	});
	auto const lowest([](unsigned set) -> unsigned { return set & (0u - set); });
	auto const class_of([](unsigned one_hot) -> std::uint32_t { return 1 == one_hot ? 0 : 2 == one_hot ? 1 : 4 == one_hot ? 2 : 3; });
	u64 const root(2 * n - 3);
	std::fill(branch_changes, branch_changes + root, 0u);
	std::vector<unsigned char> set(root + 1), state(root + 1);
	u64 total(0);
	for (u64 site(0); site < n_sites; ++site) {
		unsigned present(0);
		for (u64 leaf(0); leaf < n; ++leaf) {
			set[leaf] = (unsigned char) leaf_set(bytes[leaf * pitch + site]);
			if (0xF != set[leaf]) present |= set[leaf];
		}
		std::uint32_t steps(0);
		for (u64 t(0); t < n - 2; ++t) {
			unsigned x(set[nodes[t].a] & set[nodes[t].b]);
			if (!x) { x = set[nodes[t].a] | set[nodes[t].b]; ++steps; }
			if (t == n - 3) {
				unsigned const y(x & set[nodes[t].c]);
				if (y) x = y; else ++steps;
			}
			set[n + t] = (unsigned char) x;
		}
		sites[site] = v2m_parsimony_site{steps, present};
		state[root] = (unsigned char) lowest(set[root]);
		for (u64 t(n - 2); t-- > 0;) {
			unsigned const parent(state[n + t]);
			for (int k(0); k < (t == n - 3 ? 3 : 2); ++k) {
				u64 const x(0 == k ? nodes[t].a : 1 == k ? nodes[t].b : nodes[t].c);
				state[x] = (unsigned char) ((set[x] & parent) ? parent : lowest(set[x]));
				if (state[x] == parent) continue;
				if (mutations && total < capacity) mutations[total] = v2m_tree_mutation{std::uint32_t(site), std::uint32_t(x), class_of(parent), class_of(state[x])};
				++total;
				++branch_changes[x];
			}
		}
	}
	return total;
}


std::string nj_newick_parsimony_text(v2m_nj_node const *nodes, u64 n_leaves, std::vector<std::string> const &labels, std::uint32_t const *branch_changes)
{
	if (!branch_changes) throw std::invalid_argument("branch_changes is NULL");
	return newick_text(nodes, n_leaves, labels, nullptr, branch_changes);
}


std::string tree_mutations_text(v2m_tree_mutation const *mutations, u64 n_mutations, v2m_tree_site const *sites, u64 n_sites, std::vector<std::string> const &labels,
	u64 const *reference_positions, u64 const *aligned_positions, u64 node_count)
{
	static char const letters[] = "ACGT";
	u64 const n(labels.size());
	std::string text;
	u64 node(0);
	for (u64 i(0); i < n_mutations; ++i) {
		v2m_tree_mutation const &m(mutations[i]);
		if (m.site >= n_sites) throw std::runtime_error("mutation " + std::to_string(i) + " names site " + std::to_string(m.site) + " of " + std::to_string(n_sites));
		if (n < 3 || m.node >= 2 * n - 3 || m.from > 3 || m.to > 3) throw std::runtime_error("mutation " + std::to_string(i) + " names no branch or no class");
		if (m.node < n) {
			for (char const c : labels[m.node]) if ('\t' == c || '\n' == c || '\r' == c) throw std::runtime_error("a label holds a tab or a line break");
			text += labels[m.node];
		}
		else text += "node" + std::to_string(m.node - n);
		text += '\t';
		append_column_and_position(text, sites[m.site].column, reference_positions, aligned_positions, node_count, node);
		text += '\t';
		text += letters[m.from];
		text += '\t';
		text += letters[m.to];
		text += '\n';
	}
	return text;
}


std::string tree_sites_text(v2m_tree_site const *sites, u64 n_sites, u64 const *reference_positions, u64 const *aligned_positions, u64 node_count)
{
	static char const letters[] = "ACGT";
	std::string text;
	u64 node(0);
	for (u64 i(0); i < n_sites; ++i) {
		v2m_tree_site const &site(sites[i]);
		append_column_and_position(text, site.column, reference_positions, aligned_positions, node_count, node);
		text += '\t';
		int present(0);
		for (int k(0); k < 4; ++k) if (site.present >> k & 1) { text += letters[k]; ++present; }
		text += '\t';
		text += std::to_string(site.steps);
		text += '\t';
		text += std::to_string(std::int64_t(site.steps) - (present - 1));
		text += '\n';
	}
	return text;
}


namespace {
	struct tree_parsimony_state {
		std::vector<v2m_tree_site> sites;
		std::vector<v2m_tree_mutation> mutations;
		bool keep_mutations;
		std::exception_ptr error;
	};

	int tree_parsimony_sites_sink(void *user, v2m_tree_site const *sites, uint64_t n)
	{
		auto &st(*static_cast<tree_parsimony_state *>(user));
		try {
			st.sites.assign(sites, sites + n);
			return 0;
		} catch (...) {   // nothing may cross the C boundary
			st.error = std::current_exception();
			return 1;
		}
	}

	int tree_parsimony_mutations_sink(void *user, v2m_tree_mutation const *mutations, uint64_t n)
	{
		auto &st(*static_cast<tree_parsimony_state *>(user));
		try {
			st.mutations.insert(st.mutations.end(), mutations, mutations + n);
			return 0;
		} catch (...) {
			st.error = std::current_exception();
			return 1;
		}
	}
}


void output::output_tree_parsimony(variant_graph const &graph, std::ostream *newick, std::ostream *mutations, std::ostream *sites, bool verbose)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-tree-parsimony needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-tree-parsimony needs every chromosome copy on one GPU context");
	row_set const rows(chain_rows(graph));   // (the rows and names of output_tree())
	v2m_row_batch batch{};
	batch.n_rows = rows.copy_index.size();
	batch.copy_index = rows.copy_index.data();
	if (rows.any_cuts) {
		batch.cut_offsets = rows.cut_offsets.data();
		batch.cut_nodes = rows.cut_nodes.data();
		batch.cut_copies = rows.cut_copies.data();
	}
	if (batch.n_rows < 3 || m_tree_nodes.size() != batch.n_rows - 2) throw std::runtime_error("the parsimony outputs need the tree of output_tree() for the same rows");
	std::vector<std::uint32_t> branch_changes(2 * batch.n_rows - 3);
	tree_parsimony_state st{};
	v2m_tree_parsimony_info info{};
	// the mutations name their sites by index: the site records are needed for either text
	int const rc(v2m_tree_parsimony(m_gpu.get(), &batch, m_tree_nodes.data(), 0, branch_changes.data(), (mutations || sites) ? tree_parsimony_sites_sink : nullptr,
		mutations ? tree_parsimony_mutations_sink : nullptr, &st, &info));
	if (st.error) std::rethrow_exception(st.error);
	m_gpu.check(rc);
	auto const *const ref_pos(graph.reference_positions.data());
	auto const *const aln_pos(graph.aligned_positions.data());
	if (newick) {
		std::string const text(nj_newick_parsimony_text(m_tree_nodes.data(), batch.n_rows, rows.ids, branch_changes.data()));
		newick->write(text.data(), std::streamsize(text.size()));
	}
	if (mutations) {
		std::string const text(tree_mutations_text(st.mutations.data(), st.mutations.size(), st.sites.data(), st.sites.size(), rows.ids, ref_pos, aln_pos, graph.node_count()));
		mutations->write(text.data(), std::streamsize(text.size()));
	}
	if (sites) {
		std::string const text(tree_sites_text(st.sites.data(), st.sites.size(), ref_pos, aln_pos, graph.node_count()));
		sites->write(text.data(), std::streamsize(text.size()));
	}
	if (verbose)
		std::fprintf(stderr, "Parsimony: %llu rows, %llu columns, %llu sites, %llu mutations, %llu ranges.\n", (unsigned long long) batch.n_rows, (unsigned long long) info.n_columns,
			(unsigned long long) info.n_sites, (unsigned long long) info.n_mutations, (unsigned long long) info.n_ranges);
}


void output::output_tree_parsimony(variant_graph const &graph, char const *newick_path, char const *mutations_path, char const *sites_path, bool verbose)
{
	std::ofstream streams[3];
	char const *const paths[3] = {newick_path, mutations_path, sites_path};
	for (int k(0); k < 3; ++k) {
		if (!paths[k]) continue;
		streams[k].open(paths[k], std::ios::binary | std::ios::trunc);
		if (!streams[k]) throw std::runtime_error(std::string("unable to open ") + paths[k] + " for writing");
	}
	output_tree_parsimony(graph, newick_path ? &streams[0] : nullptr, mutations_path ? &streams[1] : nullptr, sites_path ? &streams[2] : nullptr, verbose);
	for (int k(0); k < 3; ++k) {
		if (!paths[k]) continue;
		streams[k].flush();
		if (!streams[k]) throw std::runtime_error(std::string("error while writing ") + paths[k]);
	}
}


// --- window diversity ---------------------------------------------------------------------------------------

void window_diversity_cpu(unsigned char const *rows_a, u64 n_a, unsigned char const *rows_b, u64 n_b, u64 L, u64 pitch, u64 const *bounds, u64 n_bins, void *bins, u64 *sfs,
	u64 *multiallelic)
{
	if (rows_b && sfs) throw std::invalid_argument("the between form has no spectrum");
	if (pitch < L) throw std::invalid_argument("the pitch is smaller than the columns");
	for (u64 k(0); k < n_bins; ++k) if (bounds[k] > bounds[k + 1]) throw std::invalid_argument("the bounds descend");
	if (n_bins && bounds[n_bins] > L) throw std::invalid_argument("the bounds leave the columns");
	auto const tally([pitch](unsigned char const *rows, u64 n, u64 column, u64 (&count)[4]) {
		count[0] = count[1] = count[2] = count[3] = 0;
		for (u64 r(0); r < n; ++r) {
			switch (rows[r * pitch + column] | 0x20) {
				case 'a': ++count[0]; break;
				case 'c': ++count[1]; break;
				case 'g': ++count[2]; break;
				case 't': ++count[3]; break;
				default: break;
			}
		}
	});
	if (sfs) std::fill(sfs, sfs + (n_a / 2 + 1), u64(0));
	u64 many(0);
	for (u64 k(0); k < n_bins; ++k) {
		v2m_diversity_bin within{};
		v2m_diversity_between_bin between{};
		within.columns = between.columns = bounds[k + 1] - bounds[k];
		for (u64 column(bounds[k]); column < bounds[k + 1]; ++column) {
			u64 a[4], b[4];
			tally(rows_a, n_a, column, a);
			u64 const m(a[0] + a[1] + a[2] + a[3]);
			if (rows_b) {
				tally(rows_b, n_b, column, b);
				u64 const m_b(b[0] + b[1] + b[2] + b[3]);
				if (m >= 1 && m_b >= 1) ++between.called;
				between.pairs += m * m_b;
				for (int x(0); x < 4; ++x) for (int y(0); y < 4; ++y) if (x != y) between.diffs += a[x] * b[y];
				continue;
			}
			u64 squares(0);
			int letters(0);
			for (int x(0); x < 4; ++x) { squares += a[x] * a[x]; if (a[x]) ++letters; }
			u64 const diffs((m * m - squares) / 2);
			bool const complete(m == n_a && n_a >= 2);
			if (m >= 2) { ++within.called; within.pairs += m * (m - 1) / 2; }
			within.diffs += diffs;
			if (letters >= 2) ++within.segregating;
			if (complete) {
				++within.complete;
				within.complete_diffs += diffs;
				if (letters >= 2) ++within.complete_segregating;
				if (letters >= 3) ++many;
				else if (sfs) {
					std::sort(a, a + 4);   // ascending: a[3] the major count, a[2] the minor one or 0
					++sfs[a[2]];
				}
			}
		}
		if (rows_b) static_cast<v2m_diversity_between_bin *>(bins)[k] = between;
		else static_cast<v2m_diversity_bin *>(bins)[k] = within;
	}
	if (multiallelic) *multiallelic = sfs ? many : 0;
}


// The header's order, one operation per statement.  The host library is compiled with -ffp-contract=off (build.py: CXX_FLAGS): without
// it the compiler may fuse a product into the sum of a later statement where the target has a fused multiply-add.
diversity_values diversity_values_of(v2m_diversity_bin const &w, u64 n_rows)
{
	double const none(std::numeric_limits<double>::quiet_NaN());
	diversity_values out{none, none, none};
	if (w.pairs) out.pi = double(w.diffs) / double(w.pairs);
	if (n_rows < 2) return out;
	double a1(0), a2(0);
	for (u64 i(1); i < n_rows; ++i) {
		double const di = double(i);
		double const inverse = 1.0 / di;
		a1 = a1 + inverse;
		double const square = di * di;
		double const inverse_square = 1.0 / square;
		a2 = a2 + inverse_square;
	}
	double const n = double(n_rows);
	double const S = double(w.complete_segregating);
	double const theta = S / a1;
	out.theta_w = theta;
	double const n_plus = n + 1.0, n_minus = n - 1.0;
	double const three = 3.0 * n_minus;
	double const b1 = n_plus / three;
	double const nn = n * n;
	double const nn_n = nn + n;
	double const nn_n_3 = nn_n + 3.0;
	double const twice = 2.0 * nn_n_3;
	double const nine_n = 9.0 * n;
	double const nine_n_n1 = nine_n * n_minus;
	double const b2 = twice / nine_n_n1;
	double const inv_a1 = 1.0 / a1;
	double const c1 = b1 - inv_a1;
	double const n_plus_2 = n + 2.0;
	double const a1_n = a1 * n;
	double const middle = n_plus_2 / a1_n;
	double const a1_a1 = a1 * a1;
	double const tail = a2 / a1_a1;
	double const c2_head = b2 - middle;
	double const c2 = c2_head + tail;
	double const e1 = c1 / a1;
	double const e2_den = a1_a1 + a2;
	double const e2 = c2 / e2_den;
	double const n_n1 = n * n_minus;
	double const half = n_n1 / 2.0;
	double const k = double(w.complete_diffs) / half;
	double const e1_S = e1 * S;
	double const e2_S = e2 * S;
	double const S_minus = S - 1.0;
	double const e2_term = e2_S * S_minus;
	double const v = e1_S + e2_term;
	if (v > 0) {
		double const numerator = k - theta;
		double const root = std::sqrt(v);
		out.tajima_d = numerator / root;
	}
	return out;
}


divergence_values divergence_values_of(v2m_diversity_between_bin const &between, v2m_diversity_bin const &window_a, v2m_diversity_bin const &window_b)
{
	double const none(std::numeric_limits<double>::quiet_NaN());
	divergence_values out{none, none};
	if (!between.pairs) return out;
	out.dxy = double(between.diffs) / double(between.pairs);
	if (!window_a.pairs || !window_b.pairs || !(out.dxy > 0)) return out;
	double const pi_a = double(window_a.diffs) / double(window_a.pairs);
	double const pi_b = double(window_b.diffs) / double(window_b.pairs);
	double const sum = pi_a + pi_b;
	double const twice = 2.0 * out.dxy;
	double const ratio = sum / twice;
	out.fst = 1.0 - ratio;
	return out;
}


namespace {
	void append_diversity_double(std::string &text, double value)
	{
		if (value != value) { text += "\tNA"; return; }
		char buf[48];
		std::snprintf(buf, sizeof(buf), "\t%.10g", value);
		text += buf;
	}

	void check_group_name(std::string const &group)
	{
		for (char const c : group) if ('\t' == c || '\n' == c || '\r' == c) throw std::runtime_error("a group name holds a tab or a line break");
	}
}


std::string window_diversity_text(std::string const &group, u64 n, v2m_diversity_bin const *windows, u64 const *starts, u64 const *ends, u64 n_windows, bool header)
{
	check_group_name(group);
	std::string text;
	if (header) text += "#group\tstart\tend\tcolumns\tcalled\tdiffs\tpairs\tpi\tsegregating\tcomplete\ttheta_w\ttajima_d\n";
	for (u64 i(0); i < n_windows; ++i) {
		v2m_diversity_bin const &w(windows[i]);
		diversity_values const values(diversity_values_of(w, n));
		text += group;
		for (u64 const x : {starts[i], ends[i], w.columns, w.called, w.diffs, w.pairs}) { text += '\t'; text += std::to_string(x); }
		append_diversity_double(text, values.pi);
		for (u64 const x : {w.segregating, w.complete}) { text += '\t'; text += std::to_string(x); }
		append_diversity_double(text, values.theta_w);
		append_diversity_double(text, values.tajima_d);
		text += '\n';
	}
	return text;
}


std::string window_divergence_text(std::string const &group_a, std::string const &group_b, v2m_diversity_between_bin const *between, v2m_diversity_bin const *windows_a,
	v2m_diversity_bin const *windows_b, u64 const *starts, u64 const *ends, u64 n_windows, bool header)
{
	check_group_name(group_a);
	check_group_name(group_b);
	std::string text;
	if (header) text += "#group_a\tgroup_b\tstart\tend\tcolumns\tcalled\tdiffs\tpairs\tdxy\tfst\n";
	for (u64 i(0); i < n_windows; ++i) {
		v2m_diversity_between_bin const &w(between[i]);
		divergence_values const values(divergence_values_of(w, windows_a[i], windows_b[i]));
		text += group_a;
		text += '\t';
		text += group_b;
		for (u64 const x : {starts[i], ends[i], w.columns, w.called, w.diffs, w.pairs}) { text += '\t'; text += std::to_string(x); }
		append_diversity_double(text, values.dxy);
		append_diversity_double(text, values.fst);
		text += '\n';
	}
	return text;
}


std::string diversity_sfs_text(std::string const &group, u64 n, u64 const *sfs, u64 multiallelic, bool header)
{
	check_group_name(group);
	std::string text;
	if (header) text += "#group\tn\tminor_count\tcolumns\n";
	std::string const head(group + '\t' + std::to_string(n) + '\t');
	for (u64 k(0); k < n / 2 + 1; ++k) text += head + std::to_string(k) + '\t' + std::to_string(sfs[k]) + '\n';
	text += head + "multiallelic\t" + std::to_string(multiallelic) + '\n';
	return text;
}


namespace {
	// The rows of a row_set picked by index, as a batch of their own.
	struct picked_rows {
		std::vector<std::uint32_t> copy_index;
		std::vector<std::uint64_t> cut_offsets{0}, cut_nodes;
		std::vector<std::uint32_t> cut_copies;
		bool any_cuts{};
		v2m_row_batch batch() const
		{
			v2m_row_batch b{};
			b.n_rows = copy_index.size();
			b.copy_index = copy_index.data();
			if (any_cuts) { b.cut_offsets = cut_offsets.data(); b.cut_nodes = cut_nodes.data(); b.cut_copies = cut_copies.data(); }
			return b;
		}
	};

	// Device memory of v2m_alloc_output, freed with the scope.
	struct output_buffers {
		gpu_context &gpu;
		std::vector<void *> held;
		explicit output_buffers(gpu_context &g) : gpu(g) {}
		output_buffers(output_buffers const &) = delete;
		~output_buffers() { for (void *p : held) (void) v2m_free_output(gpu.get(), p); }
		void *take(u64 bytes)
		{
			void *p(nullptr);
			gpu.check(v2m_alloc_output(gpu.get(), std::max<u64>(bytes, 16), 1, &p));
			held.push_back(p);
			return p;
		}
	};

	template <typename t_record>
	std::vector<t_record> summed_windows(std::vector<t_record> const &bins, u64 width, u64 n_windows)
	{
		static_assert(0 == sizeof(t_record) % sizeof(u64));
		constexpr std::size_t fields(sizeof(t_record) / sizeof(u64));
		std::vector<t_record> out(n_windows);
		for (u64 j(0); j < n_windows; ++j) {
			u64 sums[fields] = {};
			for (u64 k(j); k < std::min<u64>(bins.size(), j + width); ++k) {
				u64 one[fields];
				std::memcpy(one, &bins[k], sizeof(t_record));
				for (std::size_t f(0); f < fields; ++f) sums[f] += one[f];
			}
			std::memcpy(&out[j], sums, sizeof(t_record));
		}
		return out;
	}
}


void output::output_diversity(variant_graph const &graph, diversity_params const &params, std::ostream *diversity, std::ostream *sfs_stream, std::ostream *divergence, bool verbose)
{
	if (!m_more_gpus.empty()) throw std::runtime_error("--output-diversity needs every chromosome copy on one GPU context");
	if (!m_copy_shards.empty() && 0 != m_copy_shards.front().first) throw std::runtime_error("--output-diversity needs every chromosome copy on one GPU context");
	if (0 == params.step || 0 == params.window || params.window % params.step) throw std::invalid_argument("--diversity-step must divide --diversity-window");
	if (params.ref_begin >= params.ref_end || params.ref_end > params.ref_len) throw std::invalid_argument("the reference range of the diversity outputs is empty or outside the reference");
	row_set const rows(chain_rows(graph));

	// the groups, in the order their names first appear
	std::vector<std::string> names;
	std::vector<std::vector<std::size_t>> members;
	if (params.groups.empty()) {
		names.push_back("all");
		members.emplace_back(rows.ids.size());
		for (std::size_t r(0); r < rows.ids.size(); ++r) members[0][r] = r;
	} else {
		std::map<std::string, std::size_t> row_of;
		for (std::size_t r(0); r < rows.ids.size(); ++r) row_of.emplace(rows.ids[r], r);
		std::set<std::string> seen;
		for (auto const &[id, group] : params.groups) {
			auto const it(row_of.find(id));
			if (row_of.end() == it) throw std::runtime_error("--diversity-groups: \"" + id + "\" names no output sequence");
			if (!seen.insert(id).second) throw std::runtime_error("--diversity-groups: \"" + id + "\" is named twice");
			auto at(std::find(names.begin(), names.end(), group));
			if (names.end() == at) {
				if (16 == names.size()) throw std::runtime_error("--diversity-groups: more than 16 groups");
				names.push_back(group);
				members.emplace_back();
				at = names.end() - 1;
			}
			members[std::size_t(at - names.begin())].push_back(it->second);
		}
		for (auto &m : members) std::sort(m.begin(), m.end());   // (the rows in output order)
	}
	std::size_t const G(names.size());
	if (divergence && G < 2) throw std::runtime_error("--output-divergence needs at least two groups");
	std::vector<picked_rows> picked(G);
	for (std::size_t g(0); g < G; ++g) {
		picked[g].any_cuts = rows.any_cuts;
		for (std::size_t const r : members[g]) {
			picked[g].copy_index.push_back(rows.copy_index[r]);
			if (rows.any_cuts) {
				for (u64 k(rows.cut_offsets[r]); k < rows.cut_offsets[r + 1]; ++k) { picked[g].cut_nodes.push_back(rows.cut_nodes[k]); picked[g].cut_copies.push_back(rows.cut_copies[k]); }
				picked[g].cut_offsets.push_back(picked[g].cut_nodes.size());
			}
		}
	}

	// the bins: one per step of reference positions, bounded by the columns of their first positions
	u64 const span(params.ref_end - params.ref_begin), n_bins((span + params.step - 1) / params.step), width(params.window / params.step);
	std::vector<u64> bounds(n_bins + 1);
	for (u64 k(0); k < n_bins; ++k) bounds[k] = columns_of_reference_range(graph, params.ref_len, params.ref_begin + k * params.step, params.ref_end).begin;
	bounds[n_bins] = columns_of_reference_range(graph, params.ref_len, params.ref_begin, params.ref_end).end;
	u64 const L(v2m_window_length(m_gpu.get()));
	if (bounds[n_bins] - bounds[0] != L) throw std::runtime_error("the view in force is not the columns of the diversity outputs' reference range");
	u64 const n_windows(n_bins >= width ? n_bins - width + 1 : 1);
	std::vector<u64> starts(n_windows), ends(n_windows);
	for (u64 j(0); j < n_windows; ++j) {
		starts[j] = params.ref_begin + j * params.step + 1;
		ends[j] = std::min(params.ref_end, params.ref_begin + j * params.step + params.window);
	}

	std::vector<std::vector<v2m_diversity_bin>> within(G, std::vector<v2m_diversity_bin>(n_bins));
	std::vector<std::vector<u64>> spectra(G);
	std::vector<u64> multiallelic(G);
	std::vector<std::vector<v2m_diversity_between_bin>> between;   // pairs (a, b), a < b, in order
	for (std::size_t g(0); g < G; ++g) spectra[g].resize(members[g].size() / 2 + 1);
	if (params.groups.empty()) {
		v2m_row_batch const batch(picked[0].batch());
		v2m_window_diversity_info info{};
		m_gpu.check(v2m_window_diversity(m_gpu.get(), &batch, nullptr, bounds.data(), n_bins, within[0].data(), spectra[0].data(), &info));
		multiallelic[0] = info.multiallelic;
	} else {
		u64 const pitch((L + 3) & ~u64(3)), table_bytes(u64(V2M_COUNT_CLASSES) * pitch * 4);
		u64 limit(u64(16) << 30);
		if (char const *const text = std::getenv("V2M_DIVERSITY_TABLE_BYTES")) limit = std::strtoull(text, nullptr, 10);
		if (G * table_bytes > limit)
			throw std::runtime_error("the counts tables of " + std::to_string(G) + " groups over " + std::to_string(L) + " columns take " + std::to_string(G * table_bytes)
				+ " bytes, more than V2M_DIVERSITY_TABLE_BYTES = " + std::to_string(limit) + ": use --region or fewer groups");
		std::vector<u64> relative(bounds);
		for (auto &b : relative) b -= bounds[0];
		output_buffers buffers(m_gpu);
		std::vector<void *> tables(G);
		u64 most(0);
		for (std::size_t g(0); g < G; ++g) {
			tables[g] = buffers.take(table_bytes);
			v2m_row_batch const batch(picked[g].batch());
			m_gpu.check(v2m_column_counts_device(m_gpu.get(), &batch, 0, tables[g], pitch));
			most = std::max<u64>(most, members[g].size());
		}
		void *const d_bins(buffers.take(n_bins * sizeof(v2m_diversity_bin)));
		void *const d_sfs(buffers.take((most / 2 + 1) * sizeof(u64)));
		for (std::size_t g(0); g < G; ++g) {
			v2m_window_diversity_info info{};
			m_gpu.check(v2m_diversity_of_counts(m_gpu.get(), tables[g], nullptr, pitch, L, members[g].size(), 0, relative.data(), n_bins, d_bins, d_sfs, &info));
			m_gpu.check(v2m_read_output(m_gpu.get(), d_bins, n_bins * sizeof(v2m_diversity_bin), within[g].data()));
			m_gpu.check(v2m_read_output(m_gpu.get(), d_sfs, spectra[g].size() * sizeof(u64), spectra[g].data()));
			multiallelic[g] = info.multiallelic;
		}
		if (divergence) {
			for (std::size_t a(0); a < G; ++a) for (std::size_t b(a + 1); b < G; ++b) {
				between.emplace_back(n_bins);
				m_gpu.check(v2m_diversity_of_counts(m_gpu.get(), tables[a], tables[b], pitch, L, members[a].size(), members[b].size(), relative.data(), n_bins, d_bins, nullptr, nullptr));
				m_gpu.check(v2m_read_output(m_gpu.get(), d_bins, n_bins * sizeof(v2m_diversity_between_bin), between.back().data()));
			}
		}
	}

	std::vector<std::vector<v2m_diversity_bin>> windows(G);
	for (std::size_t g(0); g < G; ++g) windows[g] = summed_windows(within[g], width, n_windows);
	if (diversity) {
		for (std::size_t g(0); g < G; ++g) {
			std::string const text(window_diversity_text(names[g], members[g].size(), windows[g].data(), starts.data(), ends.data(), n_windows, 0 == g));
			diversity->write(text.data(), std::streamsize(text.size()));
		}
	}
	if (sfs_stream) {
		for (std::size_t g(0); g < G; ++g) {
			std::string const text(diversity_sfs_text(names[g], members[g].size(), spectra[g].data(), multiallelic[g], 0 == g));
			sfs_stream->write(text.data(), std::streamsize(text.size()));
		}
	}
	if (divergence) {
		std::size_t pair(0);
		for (std::size_t a(0); a < G; ++a) for (std::size_t b(a + 1); b < G; ++b, ++pair) {
			auto const sums(summed_windows(between[pair], width, n_windows));
			std::string const text(window_divergence_text(names[a], names[b], sums.data(), windows[a].data(), windows[b].data(), starts.data(), ends.data(), n_windows, 0 == pair));
			divergence->write(text.data(), std::streamsize(text.size()));
		}
	}
	if (verbose)
		std::fprintf(stderr, "Diversity: %llu rows, %llu columns, %llu groups, %llu bins, %llu windows.\n", (unsigned long long) rows.ids.size(), (unsigned long long) L,
			(unsigned long long) G, (unsigned long long) n_bins, (unsigned long long) n_windows);
}


void output::output_diversity(variant_graph const &graph, diversity_params const &params, char const *diversity_path, char const *sfs_path, char const *divergence_path, bool verbose)
{
	std::ofstream streams[3];
	char const *const paths[3] = {diversity_path, sfs_path, divergence_path};
	for (int k(0); k < 3; ++k) {
		if (!paths[k]) continue;
		streams[k].open(paths[k], std::ios::binary | std::ios::trunc);
		if (!streams[k]) throw std::runtime_error(std::string("unable to open ") + paths[k] + " for writing");
	}
	output_diversity(graph, params, diversity_path ? &streams[0] : nullptr, sfs_path ? &streams[1] : nullptr, divergence_path ? &streams[2] : nullptr, verbose);
	for (int k(0); k < 3; ++k) {
		if (!paths[k]) continue;
		streams[k].flush();
		if (!streams[k]) throw std::runtime_error(std::string("error while writing ") + paths[k]);
	}
}


// --- haplotype_output (haplotype_output.cc:38-132) ------------------------------------------------------------
output::row_set haplotype_output::rows_for(variant_graph const &graph, char sep, char const *suffix)
{
	row_set rows;
	bool const a2m('\t' == sep);
	if (m_should_output_reference) {                                                // :48-59 / :87-103
		rows.ids.push_back(prefixed("REF", sep) + suffix);
		rows.copy_index.push_back(V2M_PLOIDY_MAX);
	}
	for (std::size_t sample_idx(0); sample_idx < graph.sample_names.size(); ++sample_idx) {   // :62 / :106
		auto const &sample(graph.sample_names[sample_idx]);
		for (u32 chr_copy_idx(0); chr_copy_idx < graph.sample_ploidy(sample_idx); ++chr_copy_idx) {
			m_delegate->will_handle_sample(sample, u32(sample_idx), chr_copy_idx);
			rows.ids.push_back(prefixed(sample + (a2m ? '-' : '.') + std::to_string(1 + chr_copy_idx), sep) + suffix);   // :69-72 / :117
			rows.copy_index.push_back(graph.ploidy_csum[sample_idx] + chr_copy_idx);                                // :28-31
		}
	}
	return rows;
}


void haplotype_output::output_a2m(variant_graph const &graph, std::ostream &stream)
{
	write_a2m(rows_for(graph, '\t', ""), stream);
}


void haplotype_output::output_separate(variant_graph const &graph, bool should_include_fasta_header)
{
	char const *const suffix(should_include_fasta_header ? (m_should_output_unaligned ? ".fa" : ".a2m") : "");   // :94-100
	write_separate(rows_for(graph, '.', suffix));
}


// --- founder_sequence_greedy_output (founder_sequence_greedy_output.cc:515-597) ----------------------------------
output::row_set founder_sequence_greedy_output::rows_for(char sep, char const *suffix)
{
	if (m_cut_positions.empty() || 0 != m_cut_positions.front())
		throw std::runtime_error("cut positions must start with node 0");            // asserted at founder_sequence_greedy_output.cc:101-102
	std::size_t const col_rows(m_cut_positions.size() - 1);
	if (m_assigned_samples.size() != col_rows * m_founder_count)
		throw std::runtime_error("assigned_samples must have (cut positions - 1) x founders entries");

	row_set rows;
	rows.any_cuts = true;
	if (m_should_output_reference) {                                                // :519-531
		rows.ids.push_back(prefixed("REF", sep) + suffix);
		rows.copy_index.push_back(V2M_PLOIDY_MAX);
		rows.cut_offsets.push_back(0);
	}
	// the delegate's copy switch at each cut node (:106-114): one (node, copy) pair per cut and founder -- 17 M of them at config 4,
	// written by a few threads (every founder's run of the two arrays is its own)
	rows.cut_nodes.resize(std::size_t(m_founder_count) * col_rows);
	rows.cut_copies.resize(std::size_t(m_founder_count) * col_rows);
	for (u32 col(0); col < m_founder_count; ++col) {                                // :533-549
		m_delegate->will_handle_founder_sequence(col);
		rows.ids.push_back(prefixed(std::to_string(1 + col), sep) + suffix);        // :542
		rows.copy_index.push_back(V2M_PLOIDY_MAX);
		rows.cut_offsets.push_back(std::size_t(col + 1) * col_rows);                // (cut_offsets starts out as {0}: row r's cuts are [r], [r + 1])
	}
	{
		std::atomic<u32> next(0);
		auto const work([&] {
			for (u32 col; (col = next.fetch_add(1)) < m_founder_count;) {
				std::size_t const base(std::size_t(col) * col_rows);
				for (std::size_t k(0); k < col_rows; ++k) {
					rows.cut_nodes[base + k] = m_cut_positions[k];
					rows.cut_copies[base + k] = m_assigned_samples[base + k];
				}
			}
		});
		std::vector<std::thread> pool;
		unsigned const n_threads(std::size_t(m_founder_count) * col_rows >= (std::size_t(1) << 20) ? std::min<unsigned>(8, m_founder_count) : 1u);
		for (unsigned t(1); t < n_threads; ++t) pool.emplace_back(work);
		work();
		for (auto &t : pool) t.join();
	}
	return rows;
}


void founder_sequence_greedy_output::output_a2m(variant_graph const &, std::ostream &stream)
{
	bool const timing(nullptr != std::getenv("V2M_FOUNDER_TIMING"));
	auto const t0(std::chrono::steady_clock::now());
	row_set const rows(rows_for('\t', ""));
	auto const t1(std::chrono::steady_clock::now());
	write_a2m(rows, stream);
	if (timing) std::fprintf(stderr, "[founder] output: row tables %.3f s, rows through the GPU %.3f s\n", std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count());
}


void founder_sequence_greedy_output::output_separate(variant_graph const &, bool should_include_fasta_header)
{
	char const *const suffix(should_include_fasta_header ? (m_should_output_unaligned ? ".fa" : ".a2m") : "");
	write_separate(rows_for('.', suffix));
}

} // namespace v2m::host
