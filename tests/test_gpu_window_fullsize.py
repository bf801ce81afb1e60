"""Column windows at full size (config 3: 5009 rows of 100.3 Mbases): for windows at the start, middle and end of the chromosome,
every row's window body equals the same columns of the unwindowed device rows; the REF row's unaligned window is the reference range;
a few rows against the oracle."""

import numpy as np
import pytest

import full_parity

pytestmark = pytest.mark.gpu


def test_config3_windows_against_whole_rows():
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import synth
	ds = synth.dataset("config3")
	g = ds.graph
	L = g.aligned_length
	R = len(ds.reference)
	dev = torch.device("cuda", 0)
	with v2m.Context(0) as ctx:
		ctx.upload_graph(g, ds.reference)
		thr = torch.from_numpy(ds.edge_thresholds.astype(np.int64)).to(torch.int32).to(dev)
		src = torch.empty(ds.path_rows // 64 * ds.path_cols, dtype=torch.int64, device=dev)
		torch.cuda.synchronize()
		ds.fill_paths_device(ctx.stream, src.data_ptr(), thr.data_ptr(), 0, ds.path_cols)
		ctx.bind_path_matrix_device(src.data_ptr(), ds.path_cols, ds.path_rows)
		ctx.synchronize()
		del src
		rows = [v2m.PLOIDY_MAX] + list(range(ds.n_copies))
		ranges = [(0, 100_000), (R // 2 - 50_000, R // 2 + 50_000), (R - 100_000, R)]
		windows = [g.columns_of_reference_range(s, e) for s, e in ranges]
		assert windows[0][0] == 0 and windows[-1][1] == L

		# the windowed rows, all 5009 per window, aligned and unaligned
		win_out, win_lengths = [], []
		for b, e in windows:
			ctx.set_column_window(b, e)
			pitch = ctx.min_row_pitch
			out = torch.empty(len(rows) * pitch, dtype=torch.uint8, device=dev)
			ctx.splice_rows_device(rows, out.data_ptr(), pitch)
			win_out.append((out, pitch))
			upitch = (ctx.max_unaligned_length + 255) // 256 * 256
			uout = torch.empty(4 * upitch, dtype=torch.uint8, device=dev)
			lengths = ctx.splice_rows_device(rows[:4], uout.data_ptr(), upitch, unaligned=True, want_lengths=True)
			win_lengths.append((uout, upitch, lengths))
		ctx.set_column_window(0, L)
		ctx.synchronize()

		# the same columns of the whole rows, in batches of 256 rows
		full_pitch = ctx.min_row_pitch
		batch = 256
		full = torch.empty(batch * full_pitch, dtype=torch.uint8, device=dev)
		for r0 in range(0, len(rows), batch):
			part = rows[r0:r0 + batch]
			ctx.splice_rows_device(part, full.data_ptr(), full_pitch)
			ctx.synchronize()
			view = full[:len(part) * full_pitch].view(len(part), full_pitch)
			for (b, e), (out, pitch) in zip(windows, win_out):
				got = out[r0 * pitch:(r0 + len(part)) * pitch].view(len(part), pitch)[:, :e - b]
				assert torch.equal(got, view[:, b:e]), "rows %d.. window [%d, %d)" % (r0, b, e)

		# REF's unaligned window is the reference range; a few rows against the oracle
		og = full_parity.oracle_for(ds, [0, 1, 2])
		for (s, e), (b, en), (out, pitch), (uout, upitch, lengths) in zip(ranges, windows, win_out, win_lengths):
			assert uout[:int(lengths[0])].cpu().numpy().tobytes() == ds.reference[s:e]
			assert out[:en - b].cpu().numpy().tobytes() == og.output_sequence(ds.reference)[b:en]
			for k in range(3):
				exp = og.output_sequence(ds.reference, copy_index=k)
				r = 1 + k
				assert out[r * pitch:r * pitch + en - b].cpu().numpy().tobytes() == exp[b:en]
