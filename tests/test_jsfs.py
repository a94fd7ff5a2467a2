"""`sfs --joint`: the joint site-frequency spectrum, the pairwise-difference counts and Hudson's Fst
per window and population pair (pbg_window_jsfs, include/popbam_gpu.h; DESIGN.md "Joint SFS").  The
reference has no such output, so the checker lives here: `ref_jsfs` computes cells, diffs and fst
from (types, flags) exactly as the header defines them -- integers throughout, Fst from the integers
with IEEE double operations -- and every comparison is exact (Fst: the bits where it is finite, isnan
where it is not)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import harness
from window_helpers import _argv, bits, _blocks, mask_words, _native, _pop_masks, popcount, _random_types, _wins_tensor
from window_helpers import PARTIAL_WORD_CASES, partial_rows
from popbam_amd import cli
from popbam_amd import options as opt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")
SEED = 0x15F5
COUNTED, SEG = 2, 4   # harness flags bits
F_OUTGROUP = 0x40     # PBG_F_OUTGROUP


# ---- the checker -----------------------------------------------------------------------
def pair_list(npop):
    return [(i, j) for i in range(npop) for j in range(i + 1, npop)]


def pair_offsets(pop_n):
    """off[p] of every pair i < j in lexicographic order, and off[n_pairs] = C."""
    off = [0]
    for i, j in pair_list(len(pop_n)):
        off.append(off[-1] + (pop_n[i] + 1) * (pop_n[j] + 1))
    return off


def fst_of(swi, swj, sb, ni, nj):
    """Hudson's estimator as a ratio of sums, from the integers (Python floats are IEEE doubles)."""
    if ni < 2 or nj < 2 or sb == 0:
        return float("nan")
    pw_i = float(swi) / float(ni * (ni - 1) // 2)
    pw_j = float(swj) / float(nj * (nj - 1) // 2)
    pb = float(sb) / float(ni * nj)
    return 1.0 - (0.5 * (pw_i + pw_j)) / pb


def ref_jsfs(types, flags, pop_masks, pop_n, wins, outidx=None):
    """cells[n_win, C] (int32), diffs[n_win, n_pairs, 3] (int64), fst[n_win, n_pairs] (float64)."""
    lo, hi = mask_words(types)
    seg = (np.asarray(flags) & SEG) > 0
    npop, pairs, off = len(pop_masks), pair_list(len(pop_masks)), pair_offsets(pop_n)
    cnt = []
    for pm, n in zip(pop_masks, pop_n):
        c = popcount(lo & np.uint64(pm & (2 ** 64 - 1))) + popcount(hi & np.uint64(pm >> 64))
        if outidx is not None:   # the outgroup carries the derived allele: the counts flip
            word, sh = (lo, outidx) if outidx < 64 else (hi, outidx - 64)
            c = np.where((word >> np.uint64(sh)) & np.uint64(1) > 0, n - c, c)
        cnt.append(c)
    nw = len(wins)
    cells = np.zeros((nw, off[-1]), np.int32)
    diffs = np.zeros((nw, len(pairs), 3), np.int64)
    fst = np.full((nw, len(pairs)), np.nan, np.float64)
    for w, (beg, end) in enumerate(wins):
        if beg >= end:
            continue
        at = beg + np.flatnonzero(seg[beg:end])
        for p, (i, j) in enumerate(pairs):
            ni, nj = pop_n[i], pop_n[j]
            a, b = cnt[i][at], cnt[j][at]
            cells[w, off[p]:off[p + 1]] = np.bincount(a * (nj + 1) + b, minlength=(ni + 1) * (nj + 1))
            diffs[w, p] = ((a * (ni - a)).sum(), (b * (nj - b)).sum(), (a * (nj - b) + b * (ni - a)).sum())
            fst[w, p] = fst_of(*(int(x) for x in diffs[w, p]), ni, nj)
    assert npop == 1 or cells.shape[1] > 0
    return cells, diffs, fst


def _assert_same(got, want, what=""):
    for g, w, nm in zip(got, want, ("cells", "diffs", "fst")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, nm, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            same = np.where(np.isnan(w), np.isnan(g), bits(g) == bits(w))
        else:
            same = g == w
        assert same.all(), (what, nm, np.argwhere(~same)[:5].tolist(), g[~same][:5], w[~same][:5])


# ---- CPU tests ---------------------------------------------------------------------------
def test_checker_on_a_hand_made_window():
    """Two populations of two samples (masks 0011 and 1100), cells at a * 3 + b.
    Window [0, 4): rows 0001 -> (1, 0), 0111 -> (2, 1), 1000 -> (0, 1), and 1111 not segregating.
      cells: [3] = [7] = [1] = 1.  SW_i = 1*1 + 2*0 + 0*2 = 1, SW_j = 0 + 1*1 + 1*1 = 2,
      SB = (1*2 + 0) + (2*1 + 1*0) + (0 + 1*2) = 6; pw_i = 1/1, pw_j = 2/1, pb = 6/4:
      Fst = 1 - (0.5 * 3) / 1.5 = 0.  With the outgroup at sample 3 row 1000 flips to (2, 1): cells
      [3] = 1, [7] = 2; diffs and Fst as before.
    Window [4, 6): two rows 0101 -> (1, 1), identical across the populations: SW = 2, 2, SB = 4,
      Fst = 1 - (0.5 * 4) / 1 = -1.
    Window [6, 8): rows 0011 -> (2, 0) and 1100 -> (0, 2), fixed differences only: SW = 0, 0,
      SB = 4 + 4 = 8, Fst = 1 - 0 / 2 = exactly 1.  Window (8, 8) is empty: zeros and NaN."""
    types = np.array([0b0001, 0b0111, 0b1000, 0b1111, 0b0101, 0b0101, 0b0011, 0b1100, 0b0110], np.uint64)
    flags = np.full(len(types), COUNTED | SEG, np.uint8)
    flags[3] = COUNTED
    masks, pop_n, wins = [0b0011, 0b1100], [2, 2], [(0, 4), (4, 6), (6, 8), (8, 8)]
    cells, diffs, fst = ref_jsfs(types, flags, masks, pop_n, wins)
    assert cells.shape == (4, 9) and diffs.shape == (4, 1, 3) and fst.shape == (4, 1)
    want0 = [0] * 9
    want0[3] = want0[7] = want0[1] = 1
    assert cells[0].tolist() == want0 and diffs[0, 0].tolist() == [1, 2, 6] and fst[0, 0] == 0.0
    assert cells[1].tolist() == [0, 0, 0, 0, 2, 0, 0, 0, 0] and diffs[1, 0].tolist() == [2, 2, 4] and fst[1, 0] == -1.0
    assert cells[2].tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 0] and diffs[2, 0].tolist() == [0, 0, 8] and fst[2, 0] == 1.0
    assert not cells[3].any() and not diffs[3].any() and np.isnan(fst[3, 0])
    # the flip moves cells and leaves diffs and Fst alone
    c2, d2, f2 = ref_jsfs(types, flags, masks, pop_n, wins, outidx=3)
    want0 = [0] * 9
    want0[3], want0[7] = 1, 2
    assert c2[0].tolist() == want0 and np.array_equal(d2, diffs) and np.array_equal(bits(f2), bits(fst))
    assert c2[2].tolist() == [0, 0, 0, 0, 0, 0, 2, 0, 0]   # 1100 -> (0, 2) flips to (2, 0), cell 2 * 3 + 0
    # a population of one sample has no within-population pair: NaN, and cells 2 x (n_j + 1)
    c3, d3, f3 = ref_jsfs(types, flags, [0b0001, 0b1110], [1, 3], [(0, 9)])
    assert c3.shape == (1, 8) and c3.sum() == 8 and np.isnan(f3[0, 0]) and d3[0, 0, 0] == 0
    # the pair numbering and the packed offsets
    assert pair_list(4) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert [i * (2 * 4 - i - 1) // 2 + (j - i - 1) for i, j in pair_list(4)] == list(range(6))
    assert pair_offsets([6, 6]) == [0, 49] and pair_offsets([2, 1, 3]) == [0, 6, 18, 26]
    assert pair_offsets([2] * 62 + [1, 1])[-1] == 17767


def test_joint_option_parses():
    base = ["-f", "ref.fa", "-w", "10"]
    plain = opt.parse_args("sfs", base + ["in.bam", "chr1:1-500"])
    assert plain.output == 0
    for argv in (base + ["--joint", "in.bam", "chr1:1-500"], ["--joint"] + base + ["in.bam", "chr1:1-500"],
                 base + ["in.bam", "--joint", "chr1:1-500"], base + ["in.bam", "chr1:1-500", "--joint"]):
        o = opt.parse_args("sfs", argv)
        assert o.output == 2 and (o.bamfile, o.region) == ("in.bam", "chr1:1-500") and o.win_size == plain.win_size
    for argv in (base + ["--theta", "--joint", "in.bam", "chr1"], ["--joint"] + base + ["in.bam", "chr1", "--theta"]):
        o = opt.parse_args("sfs", argv)
        assert o.output == 3 and (o.bamfile, o.region) == ("in.bam", "chr1")
    assert opt.parse_args("sfs", base + ["--theta", "in.bam", "chr1"]).output == 1
    # only sfs has it
    assert opt.parse_args("nucdiv", base + ["--joint", "in.bam", "chr1"]).output == 0
    assert opt.parse_args("ld", base + ["--joint", "in.bam", "chr1"]).output == 0


# ---- GPU tests ---------------------------------------------------------------------------
N_SITES = 32_000
SHAPES = [(12, 2), (24, 3), (48, 2), (96, 4), (30, 5)]   # row widths 2 / 4 / 8 / 16 / 4 B; an odd population count
SHAPE_IDS = [f"n{a}p{b}" for a, b in SHAPES]
LAYOUTS = ["ref10kb", "overlap", "ragged"]
_shapes = {}


def _shape(n, npops):
    """One called synthetic batch per shape, shared by the tests (read only), with one context
    without and one with PBG_F_OUTGROUP (the flag is the context's; the rows do not depend on it)."""
    if (n, npops) not in _shapes:
        import torch
        from popbam_amd import _lib, workload
        params = workload.default_params(n, npops)
        ctx = _lib.Context(params, 0)
        syn = workload.SynthPileup(ctx, N_SITES, 10, SEED + n)
        hp = workload.HotPath(ctx, syn, [(0, N_SITES)], _lib.PBG_S_SFS)
        hp.call()
        ctx.sync_check()
        torch.cuda.synchronize()
        types, flags = harness.rows_to_sites(hp.rows.cpu().numpy(), ctx.row_bytes, N_SITES, n)
        ctx_out = _lib.Context(workload.default_params(n, npops, flag=F_OUTGROUP), 0)
        _shapes[(n, npops)] = (ctx, ctx_out, params, hp.rows, types, flags)
    return _shapes[(n, npops)]


def _layout(name, n_sites):
    from popbam_amd import workload
    if name == "ref10kb":
        return workload.reference_windows(0, n_sites, 10_000)
    if name == "overlap":
        return [(s, s + 1000) for s in range(0, n_sites - 1000, 500)]   # 1 kb / 500 bp step
    rng = np.random.default_rng(7)   # test_window_stats_match_oracle's ragged layout
    cuts = np.sort(rng.choice(n_sites, 40, replace=False))
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])] + [(5, 5), (0, 1)]


def _run_jsfs(ctx, rows, n_rows, wins, outidx=0):
    from popbam_amd import workload
    j = workload.JointSfs(ctx, len(wins), outidx)
    j(rows, _wins_tensor(wins), n_rows)
    ctx.sync_check()
    return j.cells.cpu().numpy(), j.diffs.cpu().numpy(), j.fst.cpu().numpy()


def _outgroup(mode, n):
    """(use the outgroup context, outidx): none; the first sample (inside every pair with population
    0, outside the others); the last sample (inside the pairs with the last population)."""
    return {"none": (False, None), "first": (True, 0), "last": (True, n - 1)}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["none", "first", "last"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,npops", SHAPES, ids=SHAPE_IDS)
def test_jsfs_matches_the_checker_on_called_rows(gpu_lib, n, npops, layout, mode):
    ctx, ctx_out, params, rows, types, flags = _shape(n, npops)
    wins = _layout(layout, N_SITES)
    masks, pop_n = _pop_masks(params)
    flagged, outidx = _outgroup(mode, n)
    got = _run_jsfs(ctx_out if flagged else ctx, rows, N_SITES, wins, outidx or 0)
    want = ref_jsfs(types, flags, masks, pop_n, wins, outidx)
    _assert_same(got, want, (n, npops, layout, mode))
    off = pair_offsets(pop_n)
    for p, (i, j) in enumerate(pair_list(npops)):
        J = got[0][:, off[p]:off[p + 1]].reshape(len(wins), pop_n[i] + 1, pop_n[j] + 1)
        a, b = np.meshgrid(np.arange(pop_n[i] + 1), np.arange(pop_n[j] + 1), indexing="ij")
        assert J[:, a != b].sum() > 0, (i, j)   # off-diagonal cells are populated
    assert np.isfinite(got[2]).any()
    if mode != "none":   # the flip changed cells, and only cells
        plain = ref_jsfs(types, flags, masks, pop_n, wins, None)
        assert not np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1])


def _window_stats(ctx, rows, n_rows, wins, n, npops, stats, fields, outidx=0):
    from popbam_amd import _lib, workload
    out = workload.WindowOutputs(len(wins), n, npops, "cuda", ctx.sfs_stride)
    o = out.struct(fields)
    so = _lib.PbgStatOpts(stats, 1, outidx, 0)
    wt = _wins_tensor(wins)
    ctx.check(ctx.lib.pbg_window_stats(ctx.h, rows.data_ptr(), n_rows, wt.data_ptr(), len(wins), C.byref(so), C.byref(o),
                                       workload.stream_handle()), "pbg_window_stats")
    ctx.sync_check()
    return {k: out.t[k].cpu().numpy() for k in fields}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["none", "first", "last"])
@pytest.mark.parametrize("n,npops", SHAPES, ids=SHAPE_IDS)
def test_jsfs_marginals_are_the_sfs_bins(gpu_lib, n, npops, mode):
    """sum_b J[a][b] == sfs_bins[i][a] and sum_a J[a][b] == sfs_bins[j][b] for pbg_window_stats's
    bins (pinned against the oracle's calc_sfs integers) on the same rows, windows and outidx."""
    from popbam_amd import _lib
    ctx, ctx_out, params, rows, types, flags = _shape(n, npops)
    flagged, outidx = _outgroup(mode, n)
    c = ctx_out if flagged else ctx
    wins = _layout("ragged", N_SITES)
    masks, pop_n = _pop_masks(params)
    cells, _, _ = _run_jsfs(c, rows, N_SITES, wins, outidx or 0)
    st = _window_stats(c, rows, N_SITES, wins, n, npops, _lib.PBG_S_SFS, ["num_sites", "segsites", "td", "fwh", "sfs_bins"],
                       outidx or 0)
    bins = st["sfs_bins"].reshape(len(wins), npops, ctx.sfs_stride)
    off = pair_offsets(pop_n)
    for p, (i, j) in enumerate(pair_list(npops)):
        J = cells[:, off[p]:off[p + 1]].reshape(len(wins), pop_n[i] + 1, pop_n[j] + 1)
        assert np.array_equal(J.sum(axis=2), bins[:, i, :pop_n[i] + 1]), (i, j)
        assert np.array_equal(J.sum(axis=1), bins[:, j, :pop_n[j] + 1]), (i, j)
        assert np.array_equal(J.sum(axis=(1, 2)), st["segsites"]), (i, j)
    assert bins.sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,npops", SHAPES, ids=SHAPE_IDS)
def test_jsfs_diffs_are_the_nucdiv_sums(gpu_lib, n, npops):
    """On 10 kb windows no 16-bit wrap of the difference matrix can occur, so
    pi[i] * num_sites * n_i (n_i - 1) / 2 is SW_i and dxy[i, j] * num_sites * n_i n_j is SB up to the
    roundings of nucdiv's two multiplications / divisions and of the three here, 2^-53 relative
    each: within 2^-48 relative."""
    from popbam_amd import _lib
    ctx, ctx_out, params, rows, types, flags = _shape(n, npops)
    wins = _layout("ref10kb", N_SITES)
    masks, pop_n = _pop_masks(params)
    _, diffs, _ = _run_jsfs(ctx, rows, N_SITES, wins)
    st = _window_stats(ctx, rows, N_SITES, wins, n, npops, _lib.PBG_S_NUCDIV, ["num_sites", "segsites", "pi", "dxy"])
    ns = st["num_sites"].astype(np.float64)
    pi = st["pi"].reshape(len(wins), npops)
    dxy = st["dxy"].reshape(len(wins), -1)[:, :npops * (npops - 1)]
    assert (ns > 5000).all()
    for p, (i, j) in enumerate(pair_list(npops)):
        ni, nj = pop_n[i], pop_n[j]
        for got, want, what in ((pi[:, i] * ns * (ni * (ni - 1) // 2), diffs[:, p, 0], "SW_i"),
                                (pi[:, j] * ns * (nj * (nj - 1) // 2), diffs[:, p, 1], "SW_j"),
                                (dxy[:, i * npops + (j - (i + 1))] * ns * (ni * nj), diffs[:, p, 2], "SB")):
            print(n, npops, (i, j), what, got.tolist(), want.tolist())
            assert (want > 0).all(), (i, j, what)
            assert (np.abs(got - want) <= 2.0 ** -48 * want).all(), (i, j, what, got, want)


def _crafted(n, masks, types, flags, flag=0):
    """A context with the given population masks and device rows packed from (types, flags)."""
    import torch
    from popbam_amd import _lib, workload
    params = workload.default_params(n, len(masks), flag=flag)
    for i, m in enumerate(masks):
        params.set_pop_mask(i, m)
        params.pop_n[i] = bin(m).count("1")
    ctx = _lib.Context(params, 0)
    rows = torch.from_numpy(harness.rows_from_oracle(types, flags, ctx.row_bytes).copy()).cuda()
    return ctx, params, rows


CRAFTED = {"63+63": [63, 63], "120+3+3": [120, 3, 3], "64pops": [2] * 62 + [1, 1]}


@pytest.mark.gpu
@pytest.mark.parametrize("outidx", [None, 125])
@pytest.mark.parametrize("name", list(CRAFTED))
def test_jsfs_crafted_rows_of_126_samples(gpu_lib, name, outidx):
    """Every row counted and segregating, random types, n = 126: 63 + 63 (4,096 cells, a wave per
    pair), 120 + 3 + 3, and 64 populations (2,016 pairs, C = 17,767: more cells than the LDS
    histogram holds, so the pairs go in groups and the rows are streamed once per group)."""
    sizes = CRAFTED[name]
    L, n = 3000, 126
    rng = np.random.default_rng(len(sizes))
    types = _random_types(rng, L, n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    masks = _blocks(sizes)
    ctx, params, rows = _crafted(n, masks, types, flags, F_OUTGROUP if outidx is not None else 0)
    C_ = ctx.lib.pbg_jsfs_cells(ctx.h)
    assert C_ == pair_offsets(sizes)[-1] and (name != "64pops" or C_ == 17767)
    wins = [(0, L), (17, 2001), (5, 5), (2999, 3000)]
    got = _run_jsfs(ctx, rows, L, wins, outidx or 0)
    _assert_same(got, ref_jsfs(types, flags, masks, sizes, wins, outidx), name)
    assert (got[0][0].reshape(-1).sum() == L * len(pair_list(len(sizes))))
    ctx.close()


@pytest.mark.gpu
def test_jsfs_interleaved_masks_and_a_population_of_one(gpu_lib):
    """Samples 0, 2, .. 10, samples 1, 3, .. 11, and sample 12 alone: the pairs with the population
    of one have NaN Fst and 2 x (n_j + 1) cells."""
    L, n = 3000, 13
    rng = np.random.default_rng(5)
    types = _random_types(rng, L, n)
    flags = np.where(rng.random(L) < 0.3, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = [0b0010101010101, 0b1000000000000, 0b0101010101010]
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (17, 2001)]
    got = _run_jsfs(ctx, rows, L, wins)
    assert pair_offsets([6, 1, 6]) == [0, 14, 63, 77] and got[0].shape == (2, 77)
    assert np.isnan(got[2][:, 0]).all() and np.isnan(got[2][:, 2]).all() and np.isfinite(got[2][:, 1]).all()
    _assert_same(got, ref_jsfs(types, flags, masks, [6, 1, 6], wins))
    ctx.close()


@pytest.mark.gpu
def test_jsfs_one_population_writes_nothing(gpu_lib):
    import torch
    from popbam_amd import _lib, workload
    L, n = 500, 12
    types = _random_types(np.random.default_rng(1), L, n)
    ctx, params, rows = _crafted(n, [(1 << n) - 1], types, np.full(L, COUNTED | SEG, np.uint8))
    assert ctx.lib.pbg_jsfs_cells(ctx.h) == 0
    cells = torch.full((64,), -7, dtype=torch.int32, device="cuda")
    diffs = torch.full((64,), -7, dtype=torch.int64, device="cuda")
    fst = torch.full((64,), -7.0, dtype=torch.float64, device="cuda")
    o = _lib.PbgJsfsOpts(0, 0)
    out = _lib.PbgJsfsOut(cells.data_ptr(), diffs.data_ptr(), fst.data_ptr())
    wt = _wins_tensor([(0, L)])
    rc = ctx.lib.pbg_window_jsfs(ctx.h, rows.data_ptr(), L, wt.data_ptr(), 1, C.byref(o), C.byref(out), workload.stream_handle())
    assert rc == _lib.PBG_OK
    ctx.sync_check()
    assert (cells == -7).all() and (diffs == -7).all() and (fst == -7.0).all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_jsfs_partial_last_word(gpu_lib, n, words):
    """Window [3, L) with L = 64 * 5 + 3 rows that ends at n_rows: L is no multiple of the rows per
    16-byte word, and the rows sit in a larger buffer of 0xFF bytes, which would read as segregating
    rows with every sample derived.  The same with 513 words and three rows (window_helpers.py)."""
    import torch
    L, more = partial_rows(n, words)
    rng = np.random.default_rng(n)
    types = _random_types(rng, L, n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    masks = _blocks([n // 2, n - n // 2])
    ctx, params, rows = _crafted(n, masks, types, flags)
    big = torch.full((rows.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:rows.numel()] = rows
    assert words is None or L == words * (16 // ctx.row_bytes) + 3
    wins = [(3, L), (0, L), (L - 1, L)] + more
    got = _run_jsfs(ctx, big, L, wins)
    assert got[0].sum(axis=1).tolist() == [L - 3, L, 1] + [b - a for a, b in more]
    _assert_same(got, ref_jsfs(types, flags, masks, [n // 2, n - n // 2], wins))
    ctx.close()


@pytest.mark.gpu
def test_jsfs_pair_offsets(gpu_lib):
    from popbam_amd import _lib
    sizes = CRAFTED["64pops"]
    types = _random_types(np.random.default_rng(2), 16, 126)
    ctx, params, rows = _crafted(126, _blocks(sizes), types, np.full(16, COUNTED, np.uint8))
    lib, off, npop = ctx.lib, pair_offsets(sizes), len(sizes)
    assert lib.pbg_jsfs_cells(ctx.h) == off[-1] == 17767
    for i, j in pair_list(npop):
        assert lib.pbg_jsfs_pair_offset(ctx.h, i, j) == off[i * (2 * npop - i - 1) // 2 + (j - i - 1)], (i, j)
    for i, j in ((0, 0), (1, 0), (5, 5), (63, 62), (-1, 3), (0, 64), (3, 64), (64, 65), (63, 63)):
        assert lib.pbg_jsfs_pair_offset(ctx.h, i, j) == _lib.PBG_E_ARG, (i, j)
    assert lib.pbg_jsfs_pair_offset(None, 0, 1) == _lib.PBG_E_ARG and lib.pbg_jsfs_cells(None) == 0
    ctx.close()


@pytest.mark.gpu
def test_jsfs_argument_errors(gpu_lib):
    from popbam_amd import _lib, workload
    ctx, ctx_out, params, rows, types, flags = _shape(12, 2)
    wins = _wins_tensor([(0, 1000)])
    j = workload.JointSfs(ctx, 1)
    lib, s = ctx.lib, workload.stream_handle()
    r, w, o, out = rows.data_ptr(), wins.data_ptr(), C.byref(j.opts), C.byref(j.out)
    assert lib.pbg_window_jsfs(None, r, N_SITES, w, 1, o, out, s) == _lib.PBG_E_ARG
    for args in ((None, N_SITES, w, 1, o, out), (r, N_SITES, None, 1, o, out), (r, N_SITES, w, 1, None, out),
                 (r, N_SITES, w, 1, o, None)):
        assert lib.pbg_window_jsfs(ctx.h, *args, s) == _lib.PBG_E_ARG, args
        assert lib.pbg_last_error(ctx.h)
    # outidx counts only with the flag: any value without it, a sample index with it
    for outidx in (-1, 12, 1 << 20):
        assert workload.JointSfs(ctx, 1, outidx).run(rows, wins, N_SITES) == _lib.PBG_OK
        assert workload.JointSfs(ctx_out, 1, outidx).run(rows, wins, N_SITES) == _lib.PBG_E_ARG
        assert lib.pbg_last_error(ctx_out.h)
    assert workload.JointSfs(ctx_out, 1, 11).run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    ctx_out.sync_check()
    # a window past the rows is never read: an empty window's outputs, reported by pbg_check
    bad = workload.JointSfs(ctx, 2)
    assert bad.run(rows, _wins_tensor([(0, N_SITES + 1), (0, 1000)]), N_SITES) == _lib.PBG_OK
    assert lib.pbg_check(ctx.h, None) == _lib.PBG_E_RANGE
    assert not bad.cells[0].any() and bad.cells[1].sum() > 0 and np.isnan(bad.fst[0].cpu().numpy()).all()
    assert j.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()


@pytest.mark.gpu
def test_jsfs_interleaves_with_window_stats_and_decay(gpu_lib):
    """Statistics, joint spectrum, LD decay, statistics with the same pointers on one context and
    stream: each equals its own stand-alone run on a fresh context bit for bit; two jsfs runs give
    identical bytes; a NULL member of pbg_jsfs_out leaves the others correct."""
    import torch
    from popbam_amd import _lib, workload
    n, npops, L = 12, 2, 64 * 1500
    wins = [(0, L)] + workload.reference_windows(0, L, 10_000)

    def fresh():
        ctx = _lib.Context(workload.default_params(n, npops), 0)
        syn = workload.SynthPileup(ctx, L, 10, SEED)
        hp = workload.HotPath(ctx, syn, wins, _lib.PBG_S_ZNS)
        hp.call()
        ctx.sync_check()
        return ctx, hp

    def zns(hp):
        hp.out.t["ld_val"].fill_(-1.0)
        hp.out.t["ld_snps"].fill_(-1)
        hp.window_stats()

    def zns_out(hp):
        return hp.out.t["ld_snps"].cpu().numpy().copy(), bits(hp.out.t["ld_val"].cpu().numpy()).copy()

    def arrays(x, names):
        return tuple(getattr(x, k).cpu().numpy().copy() for k in names)

    JN, DN = ("cells", "diffs", "fst"), ("pairs", "r2_sum", "n_var")
    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    want_z = zns_out(hp)
    ctx.close()
    ctx, hp = fresh()
    j0 = workload.JointSfs.of(hp)
    ctx.sync_check()
    want_j = arrays(j0, JN)
    ctx.close()
    ctx, hp = fresh()
    d0 = workload.LdDecay.of(hp, 100, 100)
    ctx.sync_check()
    want_d = arrays(d0, DN)
    ctx.close()

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    first = zns_out(hp)
    zns(hp)   # a cached plan from here on
    j = workload.JointSfs(ctx, len(wins))
    j(hp.rows, hp.wins, L)
    d = workload.LdDecay(ctx, len(wins), 100, 100)
    d(hp.rows, hp.wins, L)
    zns(hp)
    ctx.sync_check()
    second = zns_out(hp)
    for got in (first, second):
        assert np.array_equal(got[0], want_z[0]) and np.array_equal(got[1], want_z[1])
    _assert_same(arrays(j, JN), want_j, "interleaved")
    for g, w_ in zip(arrays(d, DN), want_d):
        assert g.tobytes() == w_.tobytes()
    again = workload.JointSfs(ctx, len(wins))
    again(hp.rows, hp.wins, L)
    ctx.sync_check()
    for g, w_ in zip(arrays(again, JN), arrays(j, JN)):
        assert g.tobytes() == w_.tobytes()
    assert want_j[0].sum() > 1000 and np.isfinite(want_j[2]).all()
    for k, drop in enumerate(JN):   # a NULL member: the others as before, the dropped array untouched
        part = workload.JointSfs(ctx, len(wins))
        getattr(part, drop).fill_(-3)
        setattr(part.out, drop, None)
        part(hp.rows, hp.wins, L)
        ctx.sync_check()
        got = arrays(part, JN)
        for m, nm in enumerate(JN):
            if m == k:
                assert (got[m] == -3).all(), nm
            else:
                assert got[m].tobytes() == want_j[m].tobytes(), (drop, nm)
    ctx.close()


BOUNDS_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
from popbam_amd import _lib, workload
assert _lib.load().pbg_build_info() == b"bounds"
ctx = _lib.Context(workload.default_params({n}, {npops}), 0)
syn = workload.SynthPileup(ctx, {n_sites}, 10, {seed})
wins = workload.reference_windows(0, {n_sites}, 10_000)
hp = workload.HotPath(ctx, syn, wins, _lib.PBG_S_SFS)
hp.call()
ctx.sync_check()
j = workload.JointSfs.of(hp)
ctx.sync_check()
np.savez({out!r}, rows=hp.rows.cpu().numpy(), cells=j.cells.cpu().numpy(), diffs=j.diffs.cpu().numpy(), fst=j.fst.cpu().numpy())
ctx.close()
print("ok")
"""


@pytest.mark.gpu
def test_jsfs_under_the_bounds_build(gpu_lib, tmp_path):
    """The (24, 3) reference-window case through the PBG_BOUNDS build (a fresh process): the same
    rows and the checker's numbers."""
    if not os.path.exists(BOUNDS_LIB):
        pytest.skip("the bounds build is not there (make bounds)")
    n, npops = 24, 3
    ctx, ctx_out, params, rows, types, flags = _shape(n, npops)
    out = str(tmp_path / "bounds.npz")
    env = dict(os.environ, POPBAM_GPU_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-c", BOUNDS_SNIPPET.format(repo=REPO, n=n, npops=npops, n_sites=N_SITES,
                                                                   seed=SEED + n, out=out)],
                       env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    z = np.load(out)
    assert np.array_equal(z["rows"], rows.cpu().numpy())
    masks, pop_n = _pop_masks(params)
    wins = _layout("ref10kb", N_SITES)
    _assert_same((z["cells"], z["diffs"], z["fst"]), ref_jsfs(types, flags, masks, pop_n, wins), "bounds")


# ---- command lines -----------------------------------------------------------------------
def _split_joint(ext, pops):
    """The appended --joint fields of one line -> {(i, j): (fst text, [cells])}."""
    pairs = pair_list(len(pops))
    assert len(ext) == 4 * len(pairs), ext[:8]
    out = {}
    for p, (i, j) in enumerate(pairs):
        assert ext[4 * p] == f"fst[{pops[i]},{pops[j]}]:" and ext[4 * p + 2] == f"jsfs[{pops[i]},{pops[j]}]:", ext[4 * p:4 * p + 4]
        out[(i, j)] = (ext[4 * p + 1], [int(x) for x in ext[4 * p + 3].split(",")])
    return out


JOINT_CASES = [("g03_threepops", 1), ("g04_outgroup", 0), ("g15_24s3p", 22), ("g01_base", 18)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,idx", JOINT_CASES, ids=[f"{n}-{i:02d}" for n, i in JOINT_CASES])
def test_joint_command_line(gpu_lib, name, idx):
    """`popbam sfs --joint` and `sfs --theta --joint` through cli.run and the native binary: the
    same text; with the appended columns cut off, the golden text; the jsfs[..] marginals are the
    sfs[..] columns; fst[..] is the value recomputed from the printed cells, at the printed
    precision."""
    case = fixtures.load_case(name)
    cs = case["meta"]["cases"][idx]
    argv = _argv(name, cs)
    gold = fixtures.golden_text(name, cs["stdout"]).splitlines()
    texts = {}
    for extra in (["--joint"], ["--theta", "--joint"]):
        ours = cli.run(argv[0], argv[1:] + extra)
        rc, nat, err = _native(argv[:1] + extra + argv[1:])   # the tokens in front here, at the end there
        assert rc == 0, err
        assert nat == ours
        texts[len(extra)] = ours.splitlines()
    assert len(texts[1]) == len(texts[2]) == len(gold) > 0
    seen = finite = 0
    pops = None
    for gl, l1, l2 in zip(gold, texts[1], texts[2]):
        assert l1.startswith(gl + "\tfst[") and l2.startswith(gl + "\tS["), (gl, l1)
        ext1 = l1[len(gl):].split("\t")[1:]
        ext2 = l2[len(gl):].split("\t")[1:]
        npop = len([f for f in ext2 if f.startswith("sfs[")])
        assert npop >= 2 and ext2[6 * npop:] == ext1   # --theta's six fields per population come first
        pops = [re.fullmatch(r"sfs\[(.+)\]:", ext2[6 * i + 4]).group(1) for i in range(npop)]
        sfs = [[int(x) for x in ext2[6 * i + 5].split(",")] for i in range(npop)]
        for (i, j), (ftxt, cells) in _split_joint(ext1, pops).items():
            ni, nj = len(sfs[i]) - 1, len(sfs[j]) - 1
            J = np.array(cells, np.int64).reshape(ni + 1, nj + 1)
            assert J.sum(axis=1).tolist() == sfs[i] and J.sum(axis=0).tolist() == sfs[j], (i, j)
            a, b = np.meshgrid(np.arange(ni + 1), np.arange(nj + 1), indexing="ij")
            f = fst_of(int((J * a * (ni - a)).sum()), int((J * b * (nj - b)).sum()),
                       int((J * (a * (nj - b) + b * (ni - a))).sum()), ni, nj)
            assert (ftxt.strip() == "NA") if np.isnan(f) else (ftxt == "%.5f" % f), (ftxt, f)
            seen += int(J.sum())
            finite += 0 if np.isnan(f) else 1
    assert seen > 0 and finite > 0


@pytest.mark.gpu
def test_joint_with_one_population_prints_the_reference_text(gpu_lib):
    """One population has no pair: `sfs -w 1 --joint` prints exactly the reference's text
    (tests/golden/g14_onepop/out/06_sfs_w1.tsv, the reference binary's stdout for `sfs -w 1`)."""
    d = fixtures.load_case("g14_onepop")["dir"]
    gold = open(os.path.join(d, "out", "06_sfs_w1.tsv")).read()
    argv = ["sfs", "-f", os.path.join(d, "ref.fa"), "-w", "1", os.path.join(d, "in.bam"), "chr1"]
    assert cli.run(argv[0], argv[1:]) == gold
    assert cli.run(argv[0], argv[1:] + ["--joint"]) == gold
    rc, nat, err = _native(argv + ["--joint"])
    assert rc == 0 and nat == gold, err
