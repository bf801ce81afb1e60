"""Host-side mirror of the reference's output classes for this path (include/vcf2multialign/output.hh:41-130):
the row order, FASTA identifiers and '\\n' placement of haplotype_output::output_a2m
(libvcf2multialign/haplotype_output.cc:38-82) and founder_sequence_greedy_output::output_a2m
(libvcf2multialign/founder_sequence_greedy_output.cc:515-550), with every row body produced by the
GPU through v2m_splice_rows instead of output_sequence().

With bgzf=True the stream receives a BGZF file (include/v2m_hip.h, "BGZF output") whose decompressed bytes are the plain A2M:
the '>'id'\n' and '\n' around every body in stored members, the bodies as the GPU's members, then the EOF member.

With region=(s, e) every body is the column window of the 0-based half-open reference range [s, e) (include/v2m_hip.h, "column
windows"); ids and row order stay as they are."""

from .context import RowBatch, bgzf_frame_stored
from .variant_graph import PLOIDY_MAX, columns_of_reference_range


class Output:
	def __init__(self, ctx, chromosome_id=None, should_output_reference=True, should_output_unaligned=False, bgzf=False, region=None):
		self.ctx = ctx
		self.region = region   # (s, e): only the columns of the 0-based half-open reference range [s, e) (v2m_set_column_window)
		self.bgzf = bgzf
		self.chromosome_id = chromosome_id
		self.should_output_reference = should_output_reference
		self.should_output_unaligned = should_output_unaligned

	def _fasta_id(self, name):
		return ((self.chromosome_id + "\t") if self.chromosome_id else "") + name

	def _chain_name(self, name):
		return ((self.chromosome_id + ".") if self.chromosome_id else "") + name

	def _write_chains(self, stream, names, rows):
		"""One UCSC chain per row (reference -> row) from Context.row_ops, formatted by the host library (host.chain_text); the REF row has
		no chain; a row without any M op gets none either.  Returns the number of chains written."""
		from . import host
		keep = [(n, r) for n, r in zip(names, rows) if not (isinstance(r, int) and r == PLOIDY_MAX)]
		for name in [self._chain_name("REF")] + [n for n, _ in keep]:
			if any(c.isspace() for c in name):
				raise ValueError("the sequence name %r holds whitespace, which a chain cannot" % name)
		written = 0
		for i, ((name, _), (ops, length)) in enumerate(zip(keep, self.ctx.row_ops(RowBatch([r for _, r in keep])))):
			t_size = int(ops[ops[:, 0] != 1, 1].astype("u8").sum())
			text = host.chain_text(ops, self._chain_name("REF"), t_size, name, length, 1 + i)
			stream.write(text)
			written += 1 if text else 0
		return written

	def _write_paf(self, stream, names, rows):
		"""One PAF line per row (the row as query, the reference as target) from Context.row_ops(split_match=True), formatted by the host
		library (host.paf_text); rows, names and the whitespace check are those of _write_chains.  Returns the number of lines written."""
		from . import host
		keep = [(n, r) for n, r in zip(names, rows) if not (isinstance(r, int) and r == PLOIDY_MAX)]
		for name in [self._chain_name("REF")] + [n for n, _ in keep]:
			if any(c.isspace() for c in name):
				raise ValueError("the sequence name %r holds whitespace, which a PAF line cannot" % name)
		written = 0
		for (name, _), (ops, length) in zip(keep, self.ctx.row_ops(RowBatch([r for _, r in keep]), split_match=True)):
			t_size = int(ops[ops[:, 0] != 1, 1].astype("u8").sum())
			text = host.paf_text(ops, self._chain_name("REF"), t_size, name, length)
			stream.write(text)
			written += 1 if text else 0
		return written

	def _write_column_counts(self, stream, rows, graph, all_columns):
		"""--output-column-counts: the TSV of host.column_counts_text for `rows` (those of output_a2m) from Context.column_counts, over the
		region's columns when there is one (reported as absolute); variable columns only unless all_columns.  Returns the number of lines."""
		from . import host
		if self.region is not None:
			self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			columns, counts = self.ctx.column_counts(RowBatch(rows), variable_only=not all_columns)
		finally:
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		stream.write(host.column_counts_text(len(rows), columns, counts, graph.reference_positions, graph.aligned_positions))
		return len(columns)

	def _write_distances(self, stream, ids, rows, graph, acgt_only):
		"""--output-distances: the TSV of host.distances_text for `rows` (those of output_a2m, named as --output-paf names them) from
		Context.pair_distances, over the region's columns when there is one.  Returns the info of the call."""
		from . import host
		if self.region is not None:
			self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			dist, info = self.ctx.pair_distances(RowBatch(rows), acgt_only=acgt_only, info=True)
		finally:
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		stream.write(host.distances_text(ids, dist, info["n_columns"], info["n_sites"], acgt_only))
		return info

	def _write_variable_sites(self, stream, ids, rows, graph, snp_only, positions):
		"""--output-variable-sites: the FASTA of `rows` (those of output_a2m, under its names) cut down to the variable columns from
		Context.variable_sites, over the region's columns when there is one; `positions`, a stream, receives host.site_positions_text.
		Returns the info of the call."""
		from . import host
		if self.region is not None:
			self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			columns, data, info = self.ctx.variable_sites(RowBatch(rows), snp_only=snp_only, info=True)
		finally:
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		for name, body in zip(ids, data):
			stream.write(b">" + name.encode() + b"\n")
			stream.write(body.tobytes())
			stream.write(b"\n")
		if positions is not None:
			positions.write(host.site_positions_text(columns, graph.reference_positions, graph.aligned_positions))
		return info

	def _write_ld(self, stream, rows, graph, **params):
		"""--output-ld: the TSV of host.site_ld_text for `rows` (those of output_a2m) from Context.site_ld, over the region's columns when
		there is one.  Returns the info of the call."""
		from . import host
		if self.region is not None:
			self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			sites, pairs, info = self.ctx.site_ld(RowBatch(rows), info=True, **params)
		finally:
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		stream.write(host.site_ld_text(len(rows), info["n_columns"], sites, pairs, graph.reference_positions, graph.aligned_positions, **params))
		return info

	def _write_tree(self, stream, ids, rows, graph, acgt_only, bootstrap=0, seed=1, replicates_path=None):
		"""--output-tree: the Newick text of host.nj_newick_text for `rows` named `ids` from Context.nj_tree, over the region's columns
		when there is one.  bootstrap > 0 (--tree-bootstrap, --tree-seed): the text of host.nj_newick_support_text from
		Context.nj_bootstrap, and with replicates_path (--output-tree-replicates) the replicate trees into that file, a line each.
		Returns the info of the call."""
		from . import host
		if len(rows) < 3:
			raise ValueError("--output-tree needs at least three sequences (got %d)" % len(rows))
		if self.region is not None:
			self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			if bootstrap:
				keep = replicates_path is not None
				nodes, support, *trees, info = self.ctx.nj_bootstrap(RowBatch(rows), bootstrap, seed=seed, acgt_only=acgt_only, replicates=keep, info=True)
			else:
				nodes, info = self.ctx.nj_tree(RowBatch(rows), acgt_only=acgt_only, info=True)
		finally:
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		if not bootstrap:
			stream.write(host.nj_newick_text(nodes, ids))
			return info
		stream.write(host.nj_newick_support_text(nodes, ids, support))
		if replicates_path is not None:
			with open(replicates_path, "wb") as f:
				for tree in trees[0]:
					f.write(host.nj_newick_text(tree, ids))
		return info

	def _write_tree_parsimony(self, ids, rows, graph, acgt_only, parsimony, mutations, sites, bootstrap=0, seed=1):
		"""--output-tree-parsimony, --output-tree-mutations, --output-tree-sites: the texts of host.nj_newick_parsimony_text,
		host.tree_mutations_text and host.tree_sites_text (each into its stream, where one is given) from Context.tree_parsimony on the
		tree --output-tree writes for `rows` named `ids` (with bootstrap > 0 the main tree of Context.nj_bootstrap, which is the same),
		over the region's columns when there is one.  Returns the info of the parsimony call."""
		from . import host
		if len(rows) < 3:
			raise ValueError("--output-tree needs at least three sequences (got %d)" % len(rows))
		if self.region is not None:
			self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			if bootstrap:
				nodes = self.ctx.nj_bootstrap(RowBatch(rows), bootstrap, seed=seed, acgt_only=acgt_only)[0]
			else:
				nodes = self.ctx.nj_tree(RowBatch(rows), acgt_only=acgt_only)
			site_records, branch_changes, mutation_records, info = self.ctx.tree_parsimony(RowBatch(rows), nodes, info=True,
				want_sites=mutations is not None or sites is not None, want_mutations=mutations is not None)
		finally:
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		if parsimony is not None:
			parsimony.write(host.nj_newick_parsimony_text(nodes, ids, branch_changes))
		if mutations is not None:
			mutations.write(host.tree_mutations_text(mutation_records, site_records, ids, graph.reference_positions, graph.aligned_positions))
		if sites is not None:
			sites.write(host.tree_sites_text(site_records, graph.reference_positions, graph.aligned_positions))
		return info

	def _write_diversity(self, ids, rows, graph, diversity, sfs, divergence, window, step, groups):
		"""--output-diversity, --diversity-sfs, --output-divergence (each a stream, or None): the texts of host.window_diversity_text,
		host.diversity_sfs_text and host.window_divergence_text for `rows` named `ids`, over the region's reference range when there is
		one, as the C++ driver writes them (csrc/host/output.hh: output_diversity).  window, step: --diversity-window, --diversity-step
		(None: the window); groups: (id, group) pairs or a dict, None for the one group `all`.  With groups every group is counted once
		into a table of Context.alloc_output and Context.diversity_of_counts runs per group and per pair; the tables together may
		take V2M_DIVERSITY_TABLE_BYTES (environment; default 16 GiB).  Returns (group names, windows)."""
		import os
		import numpy as np
		from . import _native as N
		from . import host
		window = int(window)
		step = window if step is None else int(step)
		if window <= 0 or step <= 0 or window % step:
			raise ValueError("--diversity-step must divide --diversity-window")
		ref, aln = graph.reference_positions, graph.aligned_positions
		ref_begin, ref_end = self.region if self.region is not None else (0, int(ref[-1]))
		if groups is None:
			names, members = ["all"], [list(range(len(rows)))]
		else:
			pairs = list(groups.items()) if isinstance(groups, dict) else list(groups)
			row_of = {i: r for r, i in reversed(list(enumerate(ids)))}
			names, members, seen = [], [], set()
			for i, group in pairs:
				if i not in row_of:
					raise ValueError("--diversity-groups: \"%s\" names no output sequence" % i)
				if i in seen:
					raise ValueError("--diversity-groups: \"%s\" is named twice" % i)
				seen.add(i)
				if group not in names:
					if len(names) == 16:
						raise ValueError("--diversity-groups: more than 16 groups")
					names.append(group)
					members.append([])
				members[names.index(group)].append(row_of[i])
			members = [sorted(m) for m in members]
		G = len(names)
		if divergence is not None and G < 2:
			raise ValueError("--output-divergence needs at least two groups")
		n_bins = -(-(ref_end - ref_begin) // step)
		width = window // step
		bounds = np.array([columns_of_reference_range(ref, aln, ref_begin + k * step, ref_end)[0] for k in range(n_bins)]
			+ [columns_of_reference_range(ref, aln, ref_begin, ref_end)[1]], dtype=np.uint64)
		n_windows = n_bins - width + 1 if n_bins >= width else 1
		starts = np.array([ref_begin + j * step + 1 for j in range(n_windows)], dtype=np.uint64)
		ends = np.array([min(ref_end, ref_begin + j * step + window) for j in range(n_windows)], dtype=np.uint64)

		def summed(bins):
			out = np.zeros(n_windows, dtype=bins.dtype)
			for name in bins.dtype.names:
				for j in range(n_windows):
					out[name][j] = bins[name][j:j + width].sum(dtype=np.uint64)
			return out

		picked = [[rows[r] for r in m] for m in members]
		if self.region is not None:
			self.ctx.set_column_window(int(bounds[0]), int(bounds[-1]))
		held = []
		try:
			L = self.ctx.window_length
			within, spectra, many, between = [], [], [], {}
			if groups is None:
				bins, spectrum, info = self.ctx.window_diversity(RowBatch(picked[0]), bounds, info=True)
				within, spectra, many = [bins], [spectrum], [info["multiallelic"]]
			else:
				pitch = (L + 3) & ~3
				table_bytes = 6 * pitch * 4
				limit = int(os.environ.get("V2M_DIVERSITY_TABLE_BYTES", 16 << 30))
				if G * table_bytes > limit:
					raise ValueError("the counts tables of %d groups over %d columns take %d bytes, more than V2M_DIVERSITY_TABLE_BYTES = %d" % (G, L, G * table_bytes, limit))
				relative = bounds - bounds[0]
				tables = []
				for g in range(G):
					held.append(self.ctx.alloc_output(max(16, table_bytes), 1))
					tables.append(held[-1])
					self.ctx.column_counts_device(RowBatch(picked[g]), tables[g], pitch)
				most = max(len(m) for m in members)
				held.append(self.ctx.alloc_output(max(16, n_bins * 64), 1))
				d_bins = held[-1]
				held.append(self.ctx.alloc_output((most // 2 + 1) * 8, 1))
				d_sfs = held[-1]
				for g in range(G):
					n = len(members[g])
					info = self.ctx.diversity_of_counts(tables[g], pitch, L, n, relative, d_bins, d_sfs)
					within.append(self.ctx.read_output(d_bins, n_bins, N.DIVERSITY_BIN_DTYPE))
					spectra.append(self.ctx.read_output(d_sfs, n // 2 + 1, np.uint64))
					many.append(info["multiallelic"])
				if divergence is not None:
					for a in range(G):
						for b in range(a + 1, G):
							self.ctx.diversity_of_counts(tables[a], pitch, L, len(members[a]), relative, d_bins, None, tables[b], len(members[b]))
							between[a, b] = self.ctx.read_output(d_bins, n_bins, N.DIVERSITY_BETWEEN_BIN_DTYPE)
		finally:
			for ptr in held:
				self.ctx.free_output(ptr)
			if self.region is not None:
				self.ctx.set_column_window(0, self.ctx.aligned_length)
		windows = [summed(b) for b in within]
		if diversity is not None:
			for g in range(G):
				diversity.write(host.window_diversity_text(names[g], len(members[g]), windows[g], starts, ends, header=g == 0))
		if sfs is not None:
			for g in range(G):
				sfs.write(host.diversity_sfs_text(names[g], len(members[g]), spectra[g], many[g], header=g == 0))
		if divergence is not None:
			first = True
			for (a, b), bins in between.items():
				divergence.write(host.window_divergence_text(names[a], names[b], summed(bins), windows[a], windows[b], starts, ends, header=first))
				first = False
		return names, windows

	def _write_rows(self, stream, ids, rows, graph):
		if self.region is None:
			return self._write_bodies(stream, ids, rows)
		self.ctx.set_column_window(*columns_of_reference_range(graph.reference_positions, graph.aligned_positions, *self.region))
		try:
			return self._write_bodies(stream, ids, rows)
		finally:
			self.ctx.set_column_window(0, self.ctx.aligned_length)

	def _write_bodies(self, stream, ids, rows):
		if self.bgzf:
			def sink(i, members):
				stream.write(bgzf_frame_stored(b">" + ids[i].encode() + b"\n"))
				stream.write(members)
				stream.write(bgzf_frame_stored(b"\n"))
		else:
			def sink(i, body):
				stream.write(b">" + ids[i].encode() + b"\n")
				stream.write(body)
				stream.write(b"\n")
		self.ctx.splice_rows(RowBatch(rows), sink=sink, unaligned=self.should_output_unaligned, bgzf=self.bgzf)
		if self.bgzf:
			stream.write(bgzf_frame_stored(b""))


class HaplotypeOutput(Output):
	"""haplotype_output (output.hh:71-78).  The graph must already be uploaded to ctx."""

	def output_a2m(self, graph, stream):
		ids, rows = [], []
		if self.should_output_reference:                                  # haplotype_output.cc:48-59
			ids.append(self._fasta_id("REF"))
			rows.append(PLOIDY_MAX)
		for sample_idx, sample in enumerate(graph.sample_names):          # :62
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):   # :65
				ids.append(self._fasta_id("%s-%d" % (sample, 1 + chr_copy_idx)))     # :69-72
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)     # :28-31
		self._write_rows(stream, ids, rows, graph)
		return len(rows)

	def output_column_counts(self, graph, stream, all_columns=False):
		"""--output-column-counts for the rows of output_a2m (REF first, unless omitted)."""
		rows = [PLOIDY_MAX] if self.should_output_reference else []
		for sample_idx in range(len(graph.sample_names)):
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)
		return self._write_column_counts(stream, rows, graph, all_columns)

	def _distance_rows(self, graph):
		"""(ids, rows): the rows of output_a2m (REF first, unless omitted), named as one file per sequence would be."""
		ids, rows = ([self._chain_name("REF")], [PLOIDY_MAX]) if self.should_output_reference else ([], [])
		for sample_idx in range(len(graph.sample_names)):
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):
				ids.append(self._chain_name("%s.%d" % (graph.sample_names[sample_idx], 1 + chr_copy_idx)))
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)
		return ids, rows

	def output_diversity(self, graph, diversity=None, sfs=None, divergence=None, window=10000, step=None, groups=None):
		"""--output-diversity, --diversity-sfs and --output-divergence (each a stream, or None) for the rows of output_distances under
		its names; window, step and groups as --diversity-window, --diversity-step and --diversity-groups."""
		ids, rows = self._distance_rows(graph)
		return self._write_diversity(ids, rows, graph, diversity, sfs, divergence, window, step, groups)

	def output_distances(self, graph, stream, acgt_only=False):
		"""--output-distances for the rows of output_a2m (REF first, unless omitted), named as one file per sequence would be."""
		ids, rows = self._distance_rows(graph)
		return self._write_distances(stream, ids, rows, graph, acgt_only)

	def output_tree(self, graph, stream, acgt_only=False):
		"""--output-tree (acgt_only: --tree-acgt-only) for the rows of output_distances under its names."""
		ids, rows = self._distance_rows(graph)
		return self._write_tree(stream, ids, rows, graph, acgt_only)

	def output_tree_bootstrap(self, graph, stream, bootstrap, seed=1, replicates_path=None, acgt_only=False):
		"""--output-tree with --tree-bootstrap=bootstrap (seed: --tree-seed; replicates_path: --output-tree-replicates; acgt_only:
		--tree-acgt-only) for the rows of output_tree."""
		ids, rows = self._distance_rows(graph)
		return self._write_tree(stream, ids, rows, graph, acgt_only, int(bootstrap), seed, replicates_path)

	def output_tree_parsimony(self, graph, parsimony=None, mutations=None, sites=None, acgt_only=False, bootstrap=0, seed=1):
		"""--output-tree-parsimony, --output-tree-mutations and --output-tree-sites (each a stream, or None) on the tree output_tree
		(bootstrap > 0: output_tree_bootstrap) writes for the same rows."""
		ids, rows = self._distance_rows(graph)
		return self._write_tree_parsimony(ids, rows, graph, acgt_only, parsimony, mutations, sites, int(bootstrap), seed)

	def output_variable_sites(self, graph, stream, snp_only=False, positions=None):
		"""--output-variable-sites (with --snp-sites and --output-site-positions) for the rows of output_a2m under its names."""
		ids, rows = ([self._fasta_id("REF")], [PLOIDY_MAX]) if self.should_output_reference else ([], [])
		for sample_idx, sample in enumerate(graph.sample_names):
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):
				ids.append(self._fasta_id("%s-%d" % (sample, 1 + chr_copy_idx)))
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)
		return self._write_variable_sites(stream, ids, rows, graph, snp_only, positions)

	def output_ld(self, graph, stream, window_sites=1000, window_columns=0, min_r2=(1, 5), min_allele_count=1):
		"""--output-ld (with --ld-window, --ld-window-columns, --ld-min-r2 as a fraction and --ld-min-count) for the rows of output_a2m."""
		rows = [PLOIDY_MAX] if self.should_output_reference else []
		for sample_idx in range(len(graph.sample_names)):
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)
		return self._write_ld(stream, rows, graph, window_sites=window_sites, window_columns=window_columns, min_r2=min_r2, min_allele_count=min_allele_count)

	def output_chain(self, graph, stream):
		"""--output-chain: the chains of the rows of output_a2m (without REF), named as one file per sequence would be."""
		names, rows = [], []
		for sample_idx, sample in enumerate(graph.sample_names):
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):
				names.append(self._chain_name("%s.%d" % (sample, 1 + chr_copy_idx)))
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)
		return self._write_chains(stream, names, rows)

	def output_paf(self, graph, stream):
		"""--output-paf: one PAF line with an = / X / I / D cigar for each row output_chain gives a chain."""
		names, rows = [], []
		for sample_idx, sample in enumerate(graph.sample_names):
			for chr_copy_idx in range(graph.sample_ploidy(sample_idx)):
				names.append(self._chain_name("%s.%d" % (sample, 1 + chr_copy_idx)))
				rows.append(int(graph.ploidy_csum[sample_idx]) + chr_copy_idx)
		return self._write_paf(stream, names, rows)


class FounderSequenceGreedyOutput(Output):
	"""The output half of founder_sequence_greedy_output (output.hh:81-130): given cut positions and the
	matching matrix (found on the host), writes REF + one row per founder."""

	def output_a2m(self, graph, cut_positions, assigned_samples_column_major, stream):
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		ids, rows = [], []
		if self.should_output_reference:                                  # founder_sequence_greedy_output.cc:519-531
			ids.append(self._fasta_id("REF"))
			rows.append(PLOIDY_MAX)
		for col_idx in range(n_founders):                                 # :533-549
			ids.append(self._fasta_id(str(1 + col_idx)))
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			rows.append(list(zip(cut_positions[:-1], col)))               # delegate: switch copy at each cut node (:106-114)
		self._write_rows(stream, ids, rows, graph)
		return len(rows)

	def output_column_counts(self, graph, cut_positions, assigned_samples_column_major, stream, all_columns=False):
		"""--output-column-counts for the rows of output_a2m (REF first, unless omitted, then the founder rows)."""
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		rows = [PLOIDY_MAX] if self.should_output_reference else []
		for col_idx in range(n_founders):
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			rows.append(list(zip(cut_positions[:-1], col)))
		return self._write_column_counts(stream, rows, graph, all_columns)

	def _distance_rows(self, cut_positions, assigned_samples_column_major):
		"""(ids, rows): the rows of output_a2m (REF first, unless omitted, then the founder rows)."""
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		ids, rows = ([self._chain_name("REF")], [PLOIDY_MAX]) if self.should_output_reference else ([], [])
		for col_idx in range(n_founders):
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			ids.append(self._chain_name(str(1 + col_idx)))
			rows.append(list(zip(cut_positions[:-1], col)))
		return ids, rows

	def output_diversity(self, graph, cut_positions, assigned_samples_column_major, diversity=None, sfs=None, divergence=None, window=10000, step=None, groups=None):
		"""--output-diversity, --diversity-sfs and --output-divergence (each a stream, or None) for the rows of output_distances under
		its names; window, step and groups as --diversity-window, --diversity-step and --diversity-groups."""
		ids, rows = self._distance_rows(cut_positions, assigned_samples_column_major)
		return self._write_diversity(ids, rows, graph, diversity, sfs, divergence, window, step, groups)

	def output_distances(self, graph, cut_positions, assigned_samples_column_major, stream, acgt_only=False):
		"""--output-distances for the rows of output_a2m (REF first, unless omitted, then the founder rows)."""
		ids, rows = self._distance_rows(cut_positions, assigned_samples_column_major)
		return self._write_distances(stream, ids, rows, graph, acgt_only)

	def output_tree(self, graph, cut_positions, assigned_samples_column_major, stream, acgt_only=False):
		"""--output-tree (acgt_only: --tree-acgt-only) for the rows of output_distances under its names."""
		ids, rows = self._distance_rows(cut_positions, assigned_samples_column_major)
		return self._write_tree(stream, ids, rows, graph, acgt_only)

	def output_tree_bootstrap(self, graph, cut_positions, assigned_samples_column_major, stream, bootstrap, seed=1, replicates_path=None, acgt_only=False):
		"""--output-tree with --tree-bootstrap=bootstrap (seed: --tree-seed; replicates_path: --output-tree-replicates; acgt_only:
		--tree-acgt-only) for the rows of output_tree."""
		ids, rows = self._distance_rows(cut_positions, assigned_samples_column_major)
		return self._write_tree(stream, ids, rows, graph, acgt_only, int(bootstrap), seed, replicates_path)

	def output_tree_parsimony(self, graph, cut_positions, assigned_samples_column_major, parsimony=None, mutations=None, sites=None, acgt_only=False, bootstrap=0, seed=1):
		"""--output-tree-parsimony, --output-tree-mutations and --output-tree-sites (each a stream, or None) on the tree output_tree
		(bootstrap > 0: output_tree_bootstrap) writes for the same rows."""
		ids, rows = self._distance_rows(cut_positions, assigned_samples_column_major)
		return self._write_tree_parsimony(ids, rows, graph, acgt_only, parsimony, mutations, sites, int(bootstrap), seed)

	def output_variable_sites(self, graph, cut_positions, assigned_samples_column_major, stream, snp_only=False, positions=None):
		"""--output-variable-sites for the rows of output_a2m (REF first, unless omitted, then the founder rows) under its names."""
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		ids, rows = ([self._fasta_id("REF")], [PLOIDY_MAX]) if self.should_output_reference else ([], [])
		for col_idx in range(n_founders):
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			ids.append(self._fasta_id(str(1 + col_idx)))
			rows.append(list(zip(cut_positions[:-1], col)))
		return self._write_variable_sites(stream, ids, rows, graph, snp_only, positions)

	def output_ld(self, graph, cut_positions, assigned_samples_column_major, stream, window_sites=1000, window_columns=0, min_r2=(1, 5), min_allele_count=1):
		"""--output-ld for the rows of output_a2m (REF first, unless omitted, then the founder rows)."""
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		rows = [PLOIDY_MAX] if self.should_output_reference else []
		for col_idx in range(n_founders):
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			rows.append(list(zip(cut_positions[:-1], col)))
		return self._write_ld(stream, rows, graph, window_sites=window_sites, window_columns=window_columns, min_r2=min_r2, min_allele_count=min_allele_count)

	def output_chain(self, graph, cut_positions, assigned_samples_column_major, stream):
		"""--output-chain for the founder rows of output_a2m."""
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		names, rows = [], []
		for col_idx in range(n_founders):
			names.append(self._chain_name(str(1 + col_idx)))
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			rows.append(list(zip(cut_positions[:-1], col)))
		return self._write_chains(stream, names, rows)

	def output_paf(self, graph, cut_positions, assigned_samples_column_major, stream):
		"""--output-paf for the founder rows of output_a2m."""
		n_rows = len(cut_positions) - 1
		n_founders = len(assigned_samples_column_major) // n_rows if n_rows else 0
		names, rows = [], []
		for col_idx in range(n_founders):
			names.append(self._chain_name(str(1 + col_idx)))
			col = assigned_samples_column_major[col_idx * n_rows:(col_idx + 1) * n_rows]
			rows.append(list(zip(cut_positions[:-1], col)))
		return self._write_paf(stream, names, rows)
