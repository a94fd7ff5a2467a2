"""`ld --decay`: r^2 binned by the distance between variable sites, per window and population
(pbg_window_ld_decay, include/popbam_gpu.h; DESIGN.md "LD decay").  The reference has no such
output, so the checker lives here: `ref_decay` computes the statistic from (types, flags) exactly
as the header defines it -- the variable-site rule of calc_zns (pop_ld.cpp:201-252), r^2 from the
plain-double formula of the host table, each bin one sequential double sum in pair order -- and
every comparison of pairs, n_var and r2_sum is bitwise."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import harness
from window_helpers import bits, mask_words, _native, _pop_masks, popcount, _random_types, _wins_tensor
from popbam_amd import cli
from popbam_amd import options as opt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")
SEED = 0xDECA7
COUNTED, SEG = 2, 4   # harness flags bits


# ---- the checker -----------------------------------------------------------------------
def r2_of(m1, m2, c11, n):
    """The host r^2 table's entry (build_r2_table): plain doubles, x = count / n."""
    x0, x1, x11 = m1 / n, m2 / n, c11 / n
    return ((x11 - x0 * x1) * (x11 - x0 * x1)) / (x0 * (1. - x0) * x1 * (1. - x1))


def ref_decay(types, flags, pop_masks, pop_n, wins, bin_bp, n_bins, min_freq=1):
    """pairs[n_win, n_pops, n_bins] (int64), r2_sum (float64), n_var[n_win, n_pops] (int32)."""
    lo, hi = mask_words(types)
    seg = (np.asarray(flags) & SEG) > 0
    nw, npop = len(wins), len(pop_masks)
    pairs = np.zeros((nw, npop, n_bins), np.int64)
    r2s = np.zeros((nw, npop, n_bins), np.float64)
    nvar = np.zeros((nw, npop), np.int32)
    reach = bin_bp * n_bins   # the largest distance any bin holds
    for i, (pm, n) in enumerate(zip(pop_masks, pop_n)):
        plo, phi = np.uint64(pm & (2 ** 64 - 1)), np.uint64(pm >> 64)
        mlo, mhi = lo & plo, hi & phi
        m = popcount(mlo) + popcount(mhi)
        var = seg & (m >= min_freq) & (m <= n - min_freq)
        for w, (beg, end) in enumerate(wins):
            if beg >= end:
                continue
            v = beg + np.flatnonzero(var[beg:end])
            nvar[w, i] = len(v)
            if len(v) < 2:
                continue
            last = np.searchsorted(v, v + reach, side="right")   # pairs (a, b), a < b < last[a]
            cnt = np.maximum(last - np.arange(1, len(v) + 1), 0)
            a = np.repeat(np.arange(len(v)), cnt)
            b = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + a + 1   # a-major, b ascending
            k = (v[b] - v[a] - 1) // bin_bp
            c11 = popcount(mlo[v[a]] & mlo[v[b]]) + popcount(mhi[v[a]] & mhi[v[b]])
            r2 = r2_of(m[v[a]].astype(np.float64), m[v[b]].astype(np.float64), c11.astype(np.float64), float(n))
            for kk in np.unique(k):
                vals = r2[k == kk]   # in pair order
                pairs[w, i, kk] = len(vals)
                r2s[w, i, kk] = np.cumsum(vals)[-1] + 0.0   # a sequential sum from +0.0
    return pairs, r2s, nvar


# ---- CPU tests ---------------------------------------------------------------------------
def test_checker_on_a_hand_made_window():
    """Six variable sites among eight marked rows: row 5 is fixed in the population (m = n) and row 7
    is counted but not segregating.  Bins of 5 bases: bin 0 holds distances 1..5, bin 1 6..10."""
    L = 31
    types, flags = np.zeros(L, np.uint64), np.full(L, COUNTED, np.uint8)
    for row, t, sg in ((0, 0b0011, 1), (2, 0b0011, 1), (3, 0b0101, 1), (5, 0b1111, 1), (7, 0b0110, 0),
                       (10, 0b0001, 1), (11, 0b0111, 1), (30, 0b0011, 1)):
        types[row] = t
        flags[row] |= SEG if sg else 0
    pairs, r2s, nvar = ref_decay(types, flags, [0b1111], [4], [(0, L)], 5, 2)
    assert nvar[0, 0] == 6
    # bin 0: (0,2) (0,3) (2,3) (10,11); bin 1: (0,10) (2,10) (2,11) (3,10) (3,11); (0,11) at 11 and
    # every pair with row 30 are out of reach
    assert pairs[0, 0].tolist() == [4, 5]
    assert r2_of(2, 2, 2, 4) == 1.0 and r2_of(2, 2, 1, 4) == 0.0   # identical / independent sites
    # 1.0 + 0.0 + 0.0 + r2(0001, 0111): m1 = 1, m2 = 3, c11 = 1 -> (1/4 - 3/16)^2 / (1/4 3/4 3/4 1/4) = 1/9
    assert r2s[0, 0, 0] == ((1.0 + 0.0) + 0.0) + 0.00390625 / 0.03515625
    # a window that ends before row 10 keeps three sites, all in bin 0
    p2, _, n2 = ref_decay(types, flags, [0b1111], [4], [(0, 10), (5, 5)], 5, 2)
    assert n2[:, 0].tolist() == [3, 0] and p2[0, 0].tolist() == [3, 0] and p2[1].sum() == 0
    # min_freq 2 drops the singletons (rows 10 and 11: m = 1 and m = 3)
    _, _, n3 = ref_decay(types, flags, [0b1111], [4], [(0, L)], 5, 2, min_freq=2)
    assert n3[0, 0] == 4


def test_decay_option_parses():
    o = opt.parse_args("ld", ["-f", "ref.fa", "-w", "10", "--decay=100,50", "in.bam", "chr1:1-500"])
    assert (o.decay_bin, o.decay_bins, o.output, o.min_freq) == (100, 50, 0, 1)
    assert (o.bamfile, o.region) == ("in.bam", "chr1:1-500")
    o = opt.parse_args("ld", ["--decay=7,256", "-e", "-f", "ref.fa", "in.bam", "chr1"])   # before any option
    assert (o.decay_bin, o.decay_bins, o.min_freq) == (7, 256, 2)
    assert (o.bamfile, o.region) == ("in.bam", "chr1")
    o = opt.parse_args("ld", ["-f", "ref.fa", "in.bam", "chr1"])
    assert (o.decay_bin, o.decay_bins) == (0, 0)
    for bad in ("--decay=0,5", "--decay=5", "--decay=5,257", "--decay=x", "--decay", "--decay=5,0", "--decay=-5,5",
                "--decay=5,5,5", "--decay=2147483648,5", "--decay= 5,5"):
        with pytest.raises(opt.PopbamError, match="Not a valid decay option"):
            opt.parse_args("ld", ["-f", "ref.fa", bad, "in.bam", "chr1"])
    for o_val in ("1", "2"):
        with pytest.raises(opt.PopbamError, match="--decay needs -o 0"):
            opt.parse_args("ld", ["-f", "ref.fa", "-o", o_val, "--decay=5,5", "in.bam", "chr1"])
    with pytest.raises(opt.PopbamError, match="Not a valid output option"):   # -o 3 stays what it was
        opt.parse_args("ld", ["-f", "ref.fa", "-o", "3", "--decay=5,5", "in.bam", "chr1"])


def test_native_decay_errors_match_the_python_cli(capsys):
    d = fixtures.load_case("g01_base")["dir"]
    ref, bam = os.path.join(d, "ref.fa"), os.path.join(d, "in.bam")
    want = {"--decay=0,5": "Not a valid decay option", "--decay=5": "Not a valid decay option",
            "--decay=5,257": "Not a valid decay option", "--decay=x": "Not a valid decay option",
            "-o 1 --decay=5,5": "--decay needs -o 0"}
    for extra, msg in want.items():
        argv = ["ld", "-f", ref] + extra.split() + [bam, "chr1"]
        rc, out, err = _native(argv)
        prc = cli.main(argv)
        pe = capsys.readouterr()
        assert rc == prc == 1 and out == "" == pe.out, argv
        assert err == pe.err and msg in err, (argv, err, pe.err)


# ---- GPU tests ---------------------------------------------------------------------------
N_SITES = 32_000
SHAPES = [(12, 2), (24, 3), (48, 2), (96, 4), (40, 1)]   # row widths 2 / 4 / 8 / 16 B; (40, 1): raw one-word masks
BINS = [(100, 100), (7, 13), (1, 256), (20000, 1)]
_shapes = {}


def _shape(n, npops):
    """One context and one called synthetic batch per shape, shared by the tests (read only)."""
    if (n, npops) not in _shapes:
        import torch
        from popbam_amd import _lib, workload
        params = workload.default_params(n, npops)
        ctx = _lib.Context(params, 0)
        syn = workload.SynthPileup(ctx, N_SITES, 10, SEED + n)
        hp = workload.HotPath(ctx, syn, [(0, N_SITES)], _lib.PBG_S_ZNS)
        hp.call()
        ctx.sync_check()
        torch.cuda.synchronize()
        types, flags = harness.rows_to_sites(hp.rows.cpu().numpy(), ctx.row_bytes, N_SITES, n)
        _shapes[(n, npops)] = (ctx, params, hp.rows, types, flags)
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


def _run_decay(ctx, rows, n_rows, wins, bin_bp, n_bins, min_freq=1):
    from popbam_amd import workload
    d = workload.LdDecay(ctx, len(wins), bin_bp, n_bins, min_freq)
    d(rows, _wins_tensor(wins), n_rows)
    ctx.sync_check()
    return d.pairs.cpu().numpy(), d.r2_sum.cpu().numpy(), d.n_var.cpu().numpy()


def _assert_same(got, want, what=""):
    for g, w, nm in zip(got, want, ("pairs", "r2_sum", "n_var")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, nm)
        same = g.view(np.uint64) == w.view(np.uint64) if g.dtype == np.float64 else g == w
        assert same.all(), (what, nm, np.argwhere(~same)[:5].tolist(), g[~same][:5], w[~same][:5])


@pytest.mark.gpu
@pytest.mark.parametrize("bin_bp,n_bins", BINS)
@pytest.mark.parametrize("layout", ["ref10kb", "overlap", "ragged"])
@pytest.mark.parametrize("n,npops", SHAPES, ids=[f"n{a}p{b}" for a, b in SHAPES])
def test_decay_matches_the_checker_on_called_rows(gpu_lib, n, npops, layout, bin_bp, n_bins):
    ctx, params, rows, types, flags = _shape(n, npops)
    wins = _layout(layout, N_SITES)
    masks, pop_n = _pop_masks(params)
    got = _run_decay(ctx, rows, N_SITES, wins, bin_bp, n_bins)
    _assert_same(got, ref_decay(types, flags, masks, pop_n, wins, bin_bp, n_bins), (n, npops, layout))
    assert got[2].sum() > 50 and got[0].sum() > 0   # the batch has variable sites and pairs in reach


@pytest.mark.gpu
@pytest.mark.parametrize("bin_bp,n_bins", [(100, 100), (7, 13)])
def test_decay_min_freq_two(gpu_lib, bin_bp, n_bins):
    ctx, params, rows, types, flags = _shape(24, 3)
    wins = _layout("ragged", N_SITES)
    masks, pop_n = _pop_masks(params)
    got = _run_decay(ctx, rows, N_SITES, wins, bin_bp, n_bins, min_freq=2)
    _assert_same(got, ref_decay(types, flags, masks, pop_n, wins, bin_bp, n_bins, 2))
    assert got[2].sum() < _run_decay(ctx, rows, N_SITES, wins, bin_bp, n_bins)[2].sum()   # singletons dropped


def _crafted(n, masks, types, flags):
    """A context with the given population masks and device rows packed from (types, flags)."""
    import torch
    from popbam_amd import _lib, workload
    params = workload.default_params(n, len(masks))
    for i, m in enumerate(masks):
        params.set_pop_mask(i, m)
        params.pop_n[i] = bin(m).count("1")
    ctx = _lib.Context(params, 0)
    rows = torch.from_numpy(harness.rows_from_oracle(types, flags, ctx.row_bytes).copy()).cuda()
    return ctx, params, rows


@pytest.mark.gpu
@pytest.mark.parametrize("n,npops", [(12, 2), (40, 1), (70, 1)])
def test_decay_lists_past_the_lds_capacity(gpu_lib, n, npops):
    """One 6,000-row window whose every row is counted and segregating, random types: far more
    variable sites than the kernel keeps in LDS (1024), so the lists go to the workspace --
    compacted masks (12, 2), raw one-word masks (40, 1), raw two-word masks (70, 1)."""
    L = 6000
    rng = np.random.default_rng(n)
    types = _random_types(rng, L, n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    per = n // npops
    masks = [((1 << per) - 1) << (i * per) for i in range(npops)]
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (100, 900)]   # the second one stays in LDS
    got = _run_decay(ctx, rows, L, wins, 4, 16)
    assert got[2][0].min() > 4000
    _assert_same(got, ref_decay(types, flags, masks, [per] * npops, wins, 4, 16))
    ctx.close()


@pytest.mark.gpu
def test_decay_offsets_past_16_bits(gpu_lib):
    """A 70,000-row window with about 200 segregating rows: row offsets need more than 16 bits."""
    L, n = 70_000, 12
    rng = np.random.default_rng(3)
    types = np.zeros(L, np.uint64)
    flags = np.full(L, COUNTED, np.uint8)
    at = np.sort(rng.choice(L, 200, replace=False))
    at[0], at[-1] = 0, L - 1
    types[at] = rng.integers(1, (1 << n) - 1, len(at), dtype=np.uint64)
    flags[at] |= SEG
    masks = [0x03F, 0xFC0]
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L)]
    got = _run_decay(ctx, rows, L, wins, 1000, 70)
    assert got[0][0, :, 66:].sum() > 0   # pairs further apart than 65,536 rows
    _assert_same(got, ref_decay(types, flags, masks, [6, 6], wins, 1000, 70))
    ctx.close()


@pytest.mark.gpu
def test_decay_interleaved_populations_and_a_population_of_one(gpu_lib):
    """Samples 0, 2, .. 10, samples 1, 3, .. 11, and sample 12 alone: a population of one sample
    has no variable site (1 <= m <= 0 never holds), so all its outputs are zero."""
    L, n = 3000, 13
    rng = np.random.default_rng(5)
    types = _random_types(rng, L, n)
    flags = np.where(rng.random(L) < 0.3, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = [0b0010101010101, 0b0101010101010, 0b1000000000000]
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (17, 2001)]
    got = _run_decay(ctx, rows, L, wins, 10, 30)
    assert got[2][:, 2].tolist() == [0, 0] and got[0][:, 2].sum() == 0 and not got[1][:, 2].any()
    _assert_same(got, ref_decay(types, flags, masks, [6, 6, 1], wins, 10, 30))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [12, 24, 48, 96])
def test_decay_bin_edges_and_a_partial_last_word(gpu_lib, n):
    """Window [3, L) whose only segregating rows are its first and its last row (distance d):
    bins with n_bins * bin_bp == d hold the pair, with == d - 1 they do not.  L is no multiple of
    the rows per 16-byte word and the window ends at n_rows: the rows sit in a larger buffer whose
    bytes past them would read as segregating rows."""
    import torch
    L = 64 * 5 + 3
    types = np.zeros(L, np.uint64) if n <= 64 else np.zeros((L, 2), np.uint64)
    flags = np.full(L, COUNTED, np.uint8)
    for r in (3, L - 1):
        if n <= 64:
            types[r] = 0b0101
        else:
            types[r] = (0b0101, 1 << 20)
        flags[r] |= SEG
    masks = [(1 << n) - 1]
    ctx, params, rows = _crafted(n, masks, types, flags)
    big = torch.full((rows.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:rows.numel()] = rows
    d = L - 1 - 3
    wins = [(3, L)]
    assert d == 319 == 29 * 11 and d - 1 == 53 * 6
    for bin_bp, n_bins, inside in ((d, 1, True), (d - 1, 1, False), (29, 11, True), (53, 6, False), (1, 256, False)):
        assert (n_bins * bin_bp >= d) == inside
        got = _run_decay(ctx, big, L, wins, bin_bp, n_bins)
        assert got[2][0, 0] == 2 and got[0].sum() == (1 if inside else 0), (bin_bp, n_bins)
        if inside:
            assert got[0][0, 0, -1] == 1
        _assert_same(got, ref_decay(types, flags, masks, [n], wins, bin_bp, n_bins), (bin_bp, n_bins))
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,npops", [(12, 2), (96, 4)])
def test_decay_bins_sum_to_zns(gpu_lib, n, npops):
    """With bins that cover the window, the bins hold every pair ZnS sums: the counts add up to
    V (V - 1) / 2 and sum_k r2_sum equals ZnS's sum -- ld_val * ns (ns - 1) / 2, ns = ld_snps -- up
    to the reordering of N = V (V - 1) / 2 non-negative doubles: |difference| <= (N + 8) 2^-52 sum
    (the standard summation bound for both orders, 8 ulps for ZnS's scaling and its inverse)."""
    import torch
    from popbam_amd import _lib, workload
    ctx, params, rows, types, flags = _shape(n, npops)
    wins = workload.reference_windows(0, N_SITES, 10_000)
    wt = _wins_tensor(wins)
    out = workload.WindowOutputs(len(wins), n, npops, "cuda", ctx.sfs_stride)
    o = out.struct(["num_sites", "segsites", "ld_snps", "ld_val"])
    so = _lib.PbgStatOpts(_lib.PBG_S_ZNS, 1, 0, 0)
    ctx.check(ctx.lib.pbg_window_stats(ctx.h, rows.data_ptr(), N_SITES, wt.data_ptr(), len(wins), C.byref(so), C.byref(o),
                                       workload.stream_handle()), "pbg_window_stats")
    ctx.sync_check()
    ns = out.t["ld_snps"].cpu().numpy().reshape(len(wins), npops)
    val = out.t["ld_val"].cpu().numpy().reshape(len(wins), npops)
    for bin_bp, n_bins in ((100, 100), (20000, 1)):
        pairs, r2s, nvar = _run_decay(ctx, rows, N_SITES, wins, bin_bp, n_bins)
        for w in range(len(wins)):
            for i in range(npops):
                V = int(nvar[w, i])
                N = V * (V - 1) // 2
                assert int(pairs[w, i].sum()) == N
                if N == 0:
                    continue
                total = math.fsum(r2s[w, i].tolist())
                zns = float(val[w, i]) * (int(ns[w, i]) * (int(ns[w, i]) - 1)) / 2
                print(f"n={n} w={w} pop={i} V={V} decay={total!r} zns={zns!r} diff={abs(total - zns):.3e} "
                      f"bound={(N + 8) * 2.0 ** -52 * total:.3e}")
                assert abs(total - zns) <= (N + 8) * 2.0 ** -52 * total
        assert nvar.min() > 20


@pytest.mark.gpu
def test_decay_interleaves_with_window_stats(gpu_lib):
    """ZnS statistics, decay, ZnS statistics with the same pointers on one context and stream: both
    ZnS outputs equal a ZnS-only run's and the decay equals a decay-only run's, bit for bit; two
    decay runs give identical bits.  The long window's lists (more than 1024 variable sites) and
    the ZnS lists share the statistics workspace."""
    import torch
    from popbam_amd import _lib, workload
    n, npops, L = 12, 2, 64 * 4000
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

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    want_ns, want_val = zns_out(hp)
    ctx.close()
    ctx, hp = fresh()
    d0 = workload.LdDecay.of(hp, 100, 100)
    ctx.sync_check()
    want = (d0.pairs.cpu().numpy(), d0.r2_sum.cpu().numpy(), d0.n_var.cpu().numpy())
    assert want[2][0].min() > 1024
    ctx.close()

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    first = zns_out(hp)
    zns(hp)   # a cached plan from here on
    d = workload.LdDecay(ctx, len(wins), 100, 100)
    d(hp.rows, hp.wins, L)
    zns(hp)
    ctx.sync_check()
    second = zns_out(hp)
    for got in (first, second):
        assert np.array_equal(got[0], want_ns) and np.array_equal(got[1], want_val)
    _assert_same((d.pairs.cpu().numpy(), d.r2_sum.cpu().numpy(), d.n_var.cpu().numpy()), want)
    again = workload.LdDecay(ctx, len(wins), 100, 100)
    again(hp.rows, hp.wins, L)
    ctx.sync_check()
    _assert_same((again.pairs.cpu().numpy(), again.r2_sum.cpu().numpy(), again.n_var.cpu().numpy()), want)
    ctx.close()


@pytest.mark.gpu
def test_decay_argument_errors(gpu_lib):
    from popbam_amd import _lib, workload
    ctx, params, rows, types, flags = _shape(12, 2)
    wins = _wins_tensor([(0, 1000)])
    for bin_bp, n_bins, mf in ((0, 5, 1), (-3, 5, 1), (5, 0, 1), (5, 257, 1), (5, 5, 0), (5, 5, 3)):
        d = workload.LdDecay(ctx, 1, bin_bp, n_bins, mf)
        assert d.run(rows, wins, N_SITES) == _lib.PBG_E_ARG, (bin_bp, n_bins, mf)
        assert ctx.lib.pbg_last_error(ctx.h), (bin_bp, n_bins, mf)
    d = workload.LdDecay(ctx, 1, 5, 5)
    lib, s = ctx.lib, workload.stream_handle()
    assert lib.pbg_window_ld_decay(ctx.h, rows.data_ptr(), N_SITES, wins.data_ptr(), 1, None, C.byref(d.out), s) == _lib.PBG_E_ARG
    assert lib.pbg_window_ld_decay(ctx.h, rows.data_ptr(), N_SITES, wins.data_ptr(), 1, C.byref(d.opts), None, s) == _lib.PBG_E_ARG
    assert lib.pbg_last_error(ctx.h)
    # a window past the rows is refused on the host, before any launch
    assert d.run(rows, _wins_tensor([(0, N_SITES + 1)]), N_SITES) == _lib.PBG_E_RANGE
    assert d.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()


def _split_decay(line, pops):
    """(the reference's part of a window line, {pop: (means, pairs)})."""
    f = line.split("\t")
    at = f.index(f"decay[{pops[0]}]:")
    ext, out = f[at:], {}
    assert len(ext) == 4 * len(pops)
    for j, p in enumerate(pops):
        assert ext[4 * j] == f"decay[{p}]:" and ext[4 * j + 2] == f"pairs[{p}]:"
        out[p] = (ext[4 * j + 1].split(","), [int(x) for x in ext[4 * j + 3].split(",")])
    return "\t".join(f[:at]), out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g01_base", "g03_threepops", "g15_24s3p"])
def test_decay_command_line(gpu_lib, name):
    """`popbam ld -w 1 --decay=50,20` through cli.run and the native binary: the reference's columns
    are untouched, the appended ones hold the library's numbers for the stream's rows."""
    import torch
    from popbam_amd import _lib, engine, workload
    case = fixtures.load_case(name)
    d = case["dir"]
    base = ["ld", "-f", os.path.join(d, "ref.fa"), "-w", "1"]
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run(base[0], base[1:] + tail)
    ours = cli.run(base[0], base[1:] + ["--decay=50,20"] + tail)
    rc, nat, err = _native(base + ["--decay=50,20"] + tail)
    assert rc == 0, err
    assert nat == ours
    gold = [c for c in case["meta"]["cases"] if c["args"] == ["ld", "-w", "1"]][0]
    assert plain == fixtures.golden_text(name, gold["stdout"])
    # the library on the stream's rows and the command's windows
    st = harness.Setup(name, ["ld", "-w", "1", "--decay=50,20"], "chr1")
    assert (st.opts.decay_bin, st.opts.decay_bins) == (50, 20)
    ctx = _lib.Context(engine.make_params(st.opts, st.sm), 0)
    kb = st.kbatch
    ref = np.ascontiguousarray(kb["ref"], dtype=np.uint8)
    k = np.ascontiguousarray(kb["k"], dtype=np.uint8 if ctx.k_bytes == 1 else np.uint16)
    rq = np.ascontiguousarray(kb["rmsq"], dtype=np.uint32)
    keys = np.ascontiguousarray(kb["keys"], dtype=np.uint16)
    L = len(ref)
    cmd = engine._Cmd(st.opts, st.sm, st.chr, st.beg, st.end)
    rows = torch.zeros(L * ctx.row_bytes, dtype=torch.uint8, device="cuda")
    with _lib.Stream(ctx, [cmd.c], 0, L) as s:
        s.push(_lib.PbgPileup(L, 0, ref.ctypes.data, k.ctypes.data, rq.ctypes.data, None, keys.ctypes.data))
        s.finish()
        text = s.text(0)
        s.rows_into(rows.data_ptr(), rows.numel())
    assert text == ours
    wins = workload.reference_windows(st.beg, st.end, st.opts.win_size)
    dec = workload.LdDecay(ctx, len(wins), 50, 20)
    dec(rows, _wins_tensor(wins), L)
    ctx.sync_check()
    pairs, r2s = dec.pairs.cpu().numpy(), dec.r2_sum.cpu().numpy()
    lines, plain_lines = ours.splitlines(), plain.splitlines()
    assert len(lines) == len(plain_lines) == len(wins) > 0
    for w, (line, pl) in enumerate(zip(lines, plain_lines)):
        head, ext = _split_decay(line, st.sm.pops)
        assert head == pl
        for i, p in enumerate(st.sm.pops):
            means, cnt = ext[p]
            assert len(means) == len(cnt) == 20
            assert cnt == pairs[w, i].tolist()
            for kk in range(20):
                assert means[kk] == ("NA" if cnt[kk] == 0 else "%.5f" % (r2s[w, i, kk] / cnt[kk]))
    assert pairs.sum() > 0
    ctx.close()


BOUNDS_SNIPPET = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
import harness
from popbam_amd import _lib, workload
ctx = _lib.Context(workload.default_params({n}, 1), 0)
L = 3000
rng = np.random.default_rng(1)
types = rng.integers(1, 2 ** 12 - 1, L, dtype=np.uint64)
rows = torch.from_numpy(harness.rows_from_oracle(types, np.full(L, 6, np.uint8), ctx.row_bytes).copy()).cuda()
wins = torch.tensor([[0, L]], dtype=torch.int32).cuda()
d = workload.LdDecay(ctx, 1, 4, 16)
out = []
for mode in ("", "pool"):   # the library reads the variable at every call
    os.environ["PBG_BOUNDS_SELFTEST"] = mode
    d(rows, wins, L)
    rc = ctx.lib.pbg_check(ctx.h, None)
    out.append("%d:%s:%d" % (rc, ctx.lib.pbg_last_error(ctx.h).decode() if rc else "", int(d.n_var[0, 0])))
ctx.close()
print("|".join(out))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("n", [12, 40])
def test_decay_bounds_build_checks_the_workspace_stores(gpu_lib, n):
    """The PBG_BOUNDS build checks the decay kernel's workspace stores: clean as it is, and the
    pool positive control (half of every slice counts as outside) trips the pool check."""
    assert os.path.exists(BOUNDS_LIB), "build it with __graft_entry__.build() (make bounds)"
    env = dict(os.environ, POPBAM_GPU_LIB=BOUNDS_LIB)
    r = subprocess.run([sys.executable, "-c", BOUNDS_SNIPPET.format(repo=REPO, n=n)], env=env, capture_output=True,
                       text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    clean, pool = (x.split(":") for x in r.stdout.strip().splitlines()[-1].split("|"))
    assert clean[0] == "0" and int(clean[2]) > 1024, r.stdout
    assert pool[0] == "-6" and "statistics workspace store" in pool[1], r.stdout
