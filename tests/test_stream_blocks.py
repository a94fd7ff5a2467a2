"""The streamed extension columns across staging blocks, and more window lists than a context keeps.

format_command (popbam_amd/csrc/stream.cpp) runs the kernel of sfs --joint, sfs --dstat, haplo --hfs,
ld --rmin, haplo --nsl, haplo --xpnsl and nucdiv --snn a block of windows at a time (win_blocks, next_block,
stage_tract): the kernel gets `d_win + first` and the block's count, the device buffer is carved by the block
size, the host vectors by the count, a window is sliced out at its index inside the block, and Rmin and the
two tract tables run a block twice, the second time with the block's own largest count as stride.  Every table
here is staged in two blocks or more (stream_blocks.LAYOUT): the stream's rows are the CPU oracle's, the line
without the option's columns is the stream's line without the option, and the columns are those the table's
own checker gives on the oracle's rows.  Where the checker over every window of a table's runs would take a
test beyond a few seconds (stream_blocks.Layout.sampled; the figures are in
test_streamed_columns_across_blocks) it runs on stream_blocks.sample_windows -- every window within 16 of a
block edge or of a run's end, every 16th, at least 200 -- and every window is also compared with one direct
library call over the whole list, which has no blocks.

The eviction test opens eleven window lists on a context that keeps eight."""
import ctypes as C
import time

import numpy as np
import pytest

import harness
import stream_blocks as sb
from stream_blocks import CASES, CASE_IDS, LAYOUT, TABLES


# ---- CPU: the census and the cases' conditions ---------------------------------------------
def test_staging_constants_are_those_of_the_source():
    """kStage, kRminGuess, kNslGuess and the window lists a context keeps, read back from stream.cpp."""
    assert sb.source_constants() == (sb.K_STAGE, sb.K_RMIN_GUESS, sb.K_NSL_GUESS, sb.WIN_LISTS) == (64 << 20, 32, 256, 8)


def test_bytes_per_window():
    """The restated bytes per window on layouts small enough to count by hand, and the block edges of the
    layouts the census was written for."""
    assert sb.bytes_per_window("joint", [1, 2]) == 6 * 4 + 8                   # one pair of 2 x 3 cells
    assert sb.bytes_per_window("joint", [2, 2, 2]) == 27 * 4 + 3 * 8
    assert sb.bytes_per_window("dstat", [1, 1, 1]) == 3 * 72                   # (0,1,2), (0,2,1), (1,2,0)
    assert sb.bytes_per_window("dstat", [2] * 4) == 12 * 72
    assert sb.bytes_per_window("hfs", [5, 3]) == 2 * (5 * 4 + 4 + 40)
    assert sb.bytes_per_window("rmin", [4, 4, 4]) == 3 * (4 + 8 * 32)
    assert sb.bytes_per_window("nsl", [4, 4, 4]) == 3 * (4 + 32 * 256)
    assert sb.bytes_per_window("xpnsl", [4, 4, 4]) == 3 * (4 + 36 * 256)
    assert sb.bytes_per_window("snn", [2, 2]) == 12 + 6 * 4                    # one group, six sample pairs
    assert sb.bytes_per_window("snn", [2, 2, 2]) == 4 * 12 + 15 * 4
    edges = {("nsl", (2,) * 63): 129, ("dstat", (2,) * 21): 233, ("xpnsl", (4,) * 8): 259, ("joint", (2,) * 63): 780,
             ("hfs", (63,) + (1,) * 63): 3542, ("rmin", (1,) * 64): 4032,
             ("xpnsl", (8, 8, 8)): 2426}   # test_xpnsl_on_a_synthetic_stream[w5]'s: 3,200 windows are two blocks
    for (t, sizes), want in edges.items():
        assert sb.block_size(t, list(sizes)) == want, (t, sizes)
    assert sb.block_size("snn", [2] * 62 + [1, 1]) == 1204                     # 64 populations, 126 samples
    assert sb.block_plan("nsl", [2] * 63, 300) == (129, [(0, 129), (129, 129), (258, 42)])
    assert sb.block_plan("nsl", [2] * 63, 100) == (100, [(0, 100)])            # a list shorter than a block
    assert sb.block_plan("dstat", [2] * 21, 234) == (233, [(0, 233), (233, 1)])


def test_every_table_has_a_run_of_two_blocks():
    runs = {t: sb.counts_of(t) for t in TABLES}
    for t in TABLES:
        size = sb.block_size(t, LAYOUT[t].sizes)
        assert max(runs[t].values()) > size, t
        if t in sb.EVERY_COUNT:
            assert sorted(runs[t].values()) == [size, size + 1, 2 * size, 2 * size + 3]
    assert [t for t in TABLES if LAYOUT[t].pos0] == ["rmin", "nsl", "xpnsl", "snn"]   # rows -> contig positions


def _census(table, run):
    b = sb.batch(table)
    nw = sb.counts_of(table)[run]
    size, blocks = sb.block_plan(table, b.sizes, nw)
    return b, nw, size, blocks


@pytest.mark.parametrize("table,run", CASES, ids=CASE_IDS)
def test_case_conditions(table, run):
    """From the census and the checker on the oracle's rows alone: the run has the blocks it is named for;
    where the table has strides, the first two blocks' differ; on each side of every block edge, among the
    16 nearest windows, at least a quarter of the checker's cells are neither 0 nor NA."""
    b, nw, size, blocks = _census(table, run)
    assert size == b.size and sum(c for _, c in blocks) == nw and all(c == size for _, c in blocks[:-1])
    want = {"size": (1, size), "size+1": (2, 1), "2size": (2, size), "2size+3": (3, 3), f"size+{b.lay.k}": (2, b.lay.k)}[run]
    assert (len(blocks), blocks[-1][1]) == want
    assert b.L <= 42_000 and (nw - 1) * b.lay.W + b.lay.W - 1 <= b.L
    idx, arrays = b.checker_for(nw)
    at = {w: k for k, w in enumerate(idx)}
    live = sb.cells(table, arrays)
    for first, _ in blocks[1:]:
        for lo, hi in ((max(0, first - 16), first), (first, min(nw, first + 16))):
            rows_ = [at[w] for w in range(lo, hi)]   # every window near an edge is in the sample
            share = live[rows_].mean()
            assert share >= 0.25, (table, run, first, (lo, hi), share)
    if table in ("rmin", "nsl", "xpnsl") and len(blocks) > 1:
        strides = _strides(b, nw, blocks)
        assert strides[0] != strides[1] and min(strides[:2]) > 0, strides
        assert max(strides) < (sb.K_RMIN_GUESS if table == "rmin" else sb.K_NSL_GUESS)   # the guess sizes the block


def _strides(b, nw, blocks):
    """Per block the largest count of its windows' chains, from the checker's counts (none of the three
    tables with a stride is sampled)."""
    assert not b.lay.sampled
    cnt = sb.counts(b.table, b.checker_for(nw)[1])
    return [int(cnt[f:f + c].max()) for f, c in blocks]


# ---- GPU: every table across its blocks ----------------------------------------------------
def _first_difference(got, want):
    for k, (x, y) in enumerate(zip(got, want)):
        if x != y:
            return k, x[k - 40:k + 80], y[k - 40:k + 80]
    return min(len(got), len(want)), got[-80:], want[-80:]


@pytest.mark.gpu
@pytest.mark.parametrize("table,run", CASES, ids=CASE_IDS)
def test_streamed_columns_across_blocks(gpu_lib, table, run):
    """A streamed run of the table's command over its host pileup, pushed in three pieces, without and with
    the option: the rows are the oracle's; every line without the option's columns is the plain line; the
    columns of every checked window are the checker's on the oracle's rows.  A sampled table (joint, dstat, snn)
    has the checker on stream_blocks.sample_windows only, and every window's columns are also those of one
    direct library call over the whole list, bit for bit as printed.  The cap is lower than 20 s of CPU, so
    that no case takes more than a few seconds: measured over all windows, test_jsfs.ref_jsfs takes 17 s for
    the 5,183 windows (24 s with 63 populations of two), test_dstat.ref_dstat 12 s for the 469 windows of the
    longest run and 35 s over the four runs, test_snn.ref_snn 5 s for the 2,132 windows; on the samples 1.2 s,
    6 s (shared by the four runs) and 0.7 s."""
    from popbam_amd import _lib
    b, nw, size, blocks = _census(table, run)
    t0 = time.time()
    ctx = _lib.Context(b.params, 0)
    try:
        rows, plain, ours = sb.stream_texts(ctx, b, nw)
        ctx.sync_check()
        assert ctx.row_bytes == len(b.rows) // b.L
        bad = np.flatnonzero((rows.reshape(b.L, -1) != b.rows.reshape(b.L, -1)).any(axis=1))
        assert bad.size == 0, f"{bad.size} rows differ from the oracle's, first {bad[0]}"
        lines, plain_lines = ours.splitlines(), plain.splitlines()
        assert len(lines) == len(plain_lines) == nw
        idx, arrays = b.checker_for(nw)
        assert len(idx) == nw or (b.lay.sampled and len(b.checker_for(b.nw_max)[0]) >= 200)
        for k, w in enumerate(idx):
            want = plain_lines[w] + sb.ext_text(b, arrays, k, w)
            assert lines[w] == want, (table, run, "checker", w, blocks, _first_difference(lines[w], want))
        if b.lay.sampled:
            lib = sb.direct(ctx, b, nw)
            for w in range(nw):
                want = plain_lines[w] + sb.ext_text(b, lib, w, w)
                assert lines[w] == want, (table, run, "library", w, blocks, _first_difference(lines[w], want))
    finally:
        ctx.close()
    print(f"{table}-{run}: block {size}, blocks {[c for _, c in blocks]}, {nw} windows, {len(idx)} checked, {time.time() - t0:.1f} s")


# ---- GPU: more window lists than a context keeps ---------------------------------------------
EV_N, EV_SIZES, EV_L, EV_POS0 = 12, [6, 6], 64 * 32, 64 * 4
EV_HALF = EV_L // 2 + 1   # -w of just over half the region: one window of EV_L / 2 rows
EV_DECAY = (50, 20)
# (pbg_cmd.cmd, output, hfs, decay, -w; 0: no windows), eleven distinct window lists
EV_CMDS = [(4, 0, 0, (0, 0), 100), (6, 2, 0, (0, 0), 150), (1, 4, 0, (0, 0), 200), (5, 0, 0, EV_DECAY, 250),
           (4, 0, 0, (0, 0), 300), (6, 2, 0, (0, 0), 350), (1, 4, 0, (0, 0), 400), (5, 0, 0, EV_DECAY, 64),
           (4, 0, 0, (0, 0), 500), (5, 0, 0, EV_DECAY, 0), (6, 2, 0, (0, 0), 600)]
EV_AGAIN = (5, 0, 0, EV_DECAY, EV_HALF)   # run first and after each of the eleven
EV_MARK = {6: "\tfst[", 1: "\tnsl[", 5: "\tdecay["}   # where the option's columns begin


def _ev_batch():
    from window_edges import founder_bits, make_params
    from call_edges import edge_batch
    rng = np.random.default_rng(0xE71C7)
    bits = founder_bits(rng, EV_L, EV_N, 12, 24, 0.5)
    depth = np.where(bits > 0, rng.integers(9, 11, bits.shape), rng.integers(3, 5, bits.shape))
    raw = edge_batch(rng.integers(0, 4, EV_L), np.zeros(EV_L, np.int64), depth, bits, rng)
    params = make_params(EV_N, EV_SIZES)
    return raw, params, harness.key_batch(raw, params)


def _ev_oracle(params, raw, keep, cmd, win):
    """orc_run's text of the command without its option: the reference's columns.  The oracle takes the
    batch from position 0, so the command's positions are shifted to rows and the printed ones back."""
    c = harness.OrcCmd()
    c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq = cmd, 0, 10, 10, 1
    c.windowed, c.win_size, c.beg, c.end = (1, win, EV_POS0, EV_POS0 + EV_L) if win else (0, 0, EV_POS0, EV_POS0 + EV_L)
    c.chr_name = keep[0]
    c.sample_names = C.cast(keep[1], C.POINTER(C.c_char_p))
    c.pop_names = C.cast(keep[2], C.POINTER(C.c_char_p))
    c.refid = b"ref"
    pad = lambda a, fill: np.concatenate([np.full((EV_POS0,) + a.shape[1:], fill, a.dtype), a])   # noqa: E731
    ref, dep = np.ascontiguousarray(pad(raw["ref"], 0x80 | ord("A"))), np.ascontiguousarray(pad(raw["depth"], 0))
    rd = np.ascontiguousarray(raw["reads"])
    buf = C.create_string_buffer(1 << 22)
    r = harness.oracle().orc_run(C.byref(harness.oracle_params_from(params)), C.byref(c), EV_POS0 + EV_L, ref.ctypes.data,
                                 dep.ctypes.data, rd.ctypes.data, buf, 1 << 22)
    assert r >= 0
    return buf.value.decode()


@pytest.mark.gpu
def test_more_window_lists_than_the_context_keeps(gpu_lib):
    """Eleven commands with distinct window lists on one context, which keeps the device copies of eight
    (window_list evicts the oldest with hipFree and erases the statistics plans and the decay plans keyed on its
    pointer): nucdiv, sfs --joint, haplo --nsl and ld --decay=50,20 at different -w, one of them without
    windows, and after each of them the same `ld --decay=50,20 -w 1025` again, whose list is evicted and made
    anew on the way.  Two of the decay lists have one window over the same 2,048 rows: -w 1025 (1,024 rows, at
    most kDecayCap variable sites, no workspace) and, later, the whole region (the longest window of the run,
    more than kDecayCap variable sites in both populations: the largest workspace need of the run).  Every
    return code is 0 (the stream raises otherwise), pbg_check is clean, every text equals the same command's
    on a fresh context, and its reference columns equal the oracle's (orc_run).

    The test cannot make hipMalloc hand a freed list's address to a later list of the same n_win and n_rows,
    which is what a stale decay plan needs to go wrong, so it does not show that erasing them matters; it is
    the first test in which a context evicts a window list at all."""
    from popbam_amd import _lib
    raw, params, kb = _ev_batch()
    _, types, _, flags = harness.oracle_call(harness.oracle_params_from(params), raw)
    from window_edges import unpack
    bits, seg = unpack(types, EV_N), (flags & sb.SEG) > 0
    for lo in (0, 6):   # variable sites of each population in the whole region and in -w 1025's window
        m = bits[:, lo:lo + 6].sum(axis=1)
        var = seg & (m > 0) & (m < 6)
        assert var.sum() > sb.DECAY_CAP and EV_L // 2 <= sb.DECAY_CAP
    pops = ["p0", "p1"]
    keep = sb.names(EV_N, pops)
    assert len({w for *_, w in EV_CMDS + [EV_AGAIN]}) == 12 > sb.WIN_LISTS and max(w for *_, w in EV_CMDS + [EV_AGAIN]) < EV_L

    def run(ctx, spec):
        cmd, out, hfs, decay, win = spec
        c = sb.command(keep, cmd, out, EV_POS0, EV_POS0 + EV_L, win, hfs, decay)
        rows, (text,) = sb.run_stream(ctx, kb, EV_L, EV_N, EV_POS0, [c])
        ctx.sync_check()
        return text

    def fresh(spec):
        ctx = _lib.Context(params, 0)
        try:
            return run(ctx, spec)
        finally:
            ctx.close()

    alone = {spec: fresh(spec) for spec in EV_CMDS + [EV_AGAIN]}
    for spec, text in alone.items():   # the reference's columns are the oracle's
        cmd, out, hfs, decay, win = spec
        want = _ev_oracle(params, raw, keep, cmd, win).splitlines()
        lines = text.splitlines()
        assert len(lines) == len(want) == (((EV_L - 1) // win) if win else 1), spec
        mark = EV_MARK.get(cmd)
        assert [ln[:ln.index(mark)] if mark else ln for ln in lines] == want, spec
    assert "decay[p0]:\t0." in alone[EV_AGAIN] and "decay[p0]:\t0." in alone[EV_CMDS[9]]
    ctx = _lib.Context(params, 0)
    try:
        assert run(ctx, EV_AGAIN) == alone[EV_AGAIN]
        for k, spec in enumerate(EV_CMDS):
            assert run(ctx, spec) == alone[spec], (k, spec)
            assert run(ctx, EV_AGAIN) == alone[EV_AGAIN], (k, spec)
        for spec in EV_CMDS[:3]:   # the first lists are long gone: made anew
            assert run(ctx, spec) == alone[spec], spec
    finally:
        ctx.close()
