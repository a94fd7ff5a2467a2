"""`sfs --dstat`: Patterson's D (ABBA-BABA), f_d and f_dM per window and population triple
(pbg_window_dstat, include/popbam_gpu.h; DESIGN.md "D statistics").  The reference has no such
output, so the checker lives here: `ref_dstat` computes the six integer sums from (types, flags)
exactly as the header defines them and d, fd, fdm from those integers with Python floats (IEEE
doubles) in the header's order of operations.  Every comparison is exact: equal integers, equal bits
for finite doubles and infinities, isnan where the checker has NaN."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import harness
from window_helpers import _argv, _arrays, bits, _blocks, mask_words, _native, _pop_masks, popcount, _random_types, _wins_tensor
from window_helpers import PARTIAL_WORD_CASES, partial_rows
from popbam_amd import cli
from popbam_amd import options as opt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")
SEED = 0x15F5
COUNTED, SEG = 2, 4   # harness flags bits
F_OUTGROUP = 0x40     # PBG_F_OUTGROUP
NAMES = ("sums", "d", "fd", "fdm")


# ---- the checker -----------------------------------------------------------------------
def all_triples(npop):
    """The command line's list: (i, j, k), i < j, k neither, in lexicographic order."""
    return [(i, j, k) for i in range(npop) for j in range(i + 1, npop) for k in range(npop) if k not in (i, j)]


def ratios_of(s, n1, n2, n3):
    """d, fd, fdm from the six integers, operation by operation as the header has them."""
    s0, s1, s2, s3, s4, s5 = (int(x) for x in s)
    nan = float("nan")
    num = float(s0 - s1) / float(n1 * n2 * n3)
    den = float(s2) / float(n1 * n2 * n2) + float(s3) / float(n1 * n3 * n3)
    den2 = float(s4) / float(n2 * n1 * n1) + float(s5) / float(n2 * n3 * n3)
    d = nan if s0 + s1 == 0 else float(s0 - s1) / float(s0 + s1)
    fd = nan if den == 0.0 else num / den
    dm = den if s0 >= s1 else den2
    fdm = nan if dm == 0.0 else num / dm
    return d, fd, fdm


def derived_counts(types, pop_masks, pop_n, outidx=None):
    """[L, npop] int64: the per-population derived counts, flipped where the outgroup is derived."""
    lo, hi = mask_words(types)
    cnt = []
    for pm, n in zip(pop_masks, pop_n):
        c = popcount(lo & np.uint64(pm & (2 ** 64 - 1))) + popcount(hi & np.uint64(pm >> 64))
        if outidx is not None:
            word, sh = (lo, outidx) if outidx < 64 else (hi, outidx - 64)
            c = np.where((word >> np.uint64(sh)) & np.uint64(1) > 0, n - c, c)
        cnt.append(c)
    return np.stack(cnt, axis=1)


def ref_dstat(types, flags, pop_masks, pop_n, wins, triples, outidx=None):
    """sums[n_win, n_triples, 6] (int64) and d, fd, fdm[n_win, n_triples] (float64)."""
    cnt = derived_counts(types, pop_masks, pop_n, outidx)
    seg = (np.asarray(flags) & SEG) > 0
    tr = np.asarray(triples, np.int64).reshape(-1, 3)
    nn = np.asarray(pop_n, np.int64)
    nw, nt = len(wins), len(tr)
    sums = np.zeros((nw, nt, 6), np.int64)
    vals = np.full((3, nw, nt), np.nan, np.float64)
    for w, (beg, end) in enumerate(wins):
        at = beg + np.flatnonzero(seg[beg:end]) if beg < end else np.zeros(0, np.int64)
        cw = cnt[at]
        for t0 in range(0, nt, 256):   # a block of triples at a time: [rows, triples] arrays
            blk = tr[t0:t0 + 256]
            a, b, c = cw[:, blk[:, 0]], cw[:, blk[:, 1]], cw[:, blk[:, 2]]
            n1, n2, n3 = nn[blk[:, 0]], nn[blk[:, 1]], nn[blk[:, 2]]
            d2 = b * n3 >= c * n2   # the donor is P2 (ties here), else P3
            d1 = a * n3 >= c * n1   # the donor is P1 (ties here), else P3
            out = sums[w, t0:t0 + 256]
            out[:, 0] = ((n1 - a) * b * c).sum(axis=0)
            out[:, 1] = (a * (n2 - b) * c).sum(axis=0)
            out[:, 2] = np.where(d2, b * (b * n1 - a * n2), 0).sum(axis=0)
            out[:, 3] = np.where(d2, 0, c * (c * n1 - a * n3)).sum(axis=0)
            out[:, 4] = np.where(d1, a * (a * n2 - b * n1), 0).sum(axis=0)
            out[:, 5] = np.where(d1, 0, c * (c * n2 - b * n3)).sum(axis=0)
        for t, (p1, p2, p3) in enumerate(tr):
            vals[:, w, t] = ratios_of(sums[w, t], int(nn[p1]), int(nn[p2]), int(nn[p3]))
    return sums, vals[0], vals[1], vals[2]


def _assert_same(got, want, what=""):
    for g, w, nm in zip(got, want, NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, nm, g.shape, w.shape, g.dtype, w.dtype)
        if g.dtype == np.float64:
            same = np.where(np.isnan(w), np.isnan(g), bits(g) == bits(w))
        else:
            same = g == w
        assert same.all(), (what, nm, np.argwhere(~same)[:5].tolist(), g[~same][:5], w[~same][:5])


# ---- CPU tests ---------------------------------------------------------------------------
HAND_TYPES = [0b111100, 0b110011, 0b010101, 0b100100, 0b111111, 0b000011, 0b110100]


def test_checker_on_a_hand_made_window():
    """Three populations of two samples: P1 = samples 0, 1, P2 = 2, 3, P3 = 4, 5; every n is 2, so
    the tests are b >= c (donor P2) and a >= c (donor P1).  Rows as (a, b, c):
    Window [0, 5):
      111100 -> (0, 2, 2): ABBA 2*2*2 = 8, BABA 0; b = c, the tie is P2's: FD2 += 2*(2*2 - 0*2) = 8;
                           a < c: GD3 += 2*(2*2 - 2*2) = 0
      110011 -> (2, 0, 2): ABBA 0, BABA 2*2*2 = 8; b < c: FD3 += 2*(2*2 - 2*2) = 0; a = c, the tie is
                           P1's: GD1 += 2*(2*2 - 0*2) = 8
      010101 -> (1, 1, 1): ABBA 1, BABA 1; FD2 += 1*(1*2 - 1*2) = 0; GD1 += 0
      100100 -> (0, 1, 1): ABBA 2*1*1 = 2, BABA 0; FD2 += 1*(1*2 - 0) = 2; a < c: GD3 += 1*(1*2 - 1*2) = 0
      111111 is not segregating.
      sums 11, 9, 10, 0, 8, 0: num = 2/8, den = 10/8, den2 = 8/8; D = 2/20 = 0.1, fd = 0.25/1.25 = 0.2,
      fdM = fd since ABBA >= BABA.
      With the outgroup at sample 5 the rows with bit 5 flip: (2, 0, 0), (0, 2, 0), (1, 1, 1), (2, 1, 1):
      ABBA 0+0+1+0 = 1, BABA 0+0+1+2 = 3, FD2 0 + 2*4 + 0 + 1*(2 - 4) = 6, FD3 0, GD1 2*4 + 0 + 0 +
      2*(4 - 2) = 12, GD3 0: D = -2/4, fd = (-2/8)/(6/8) = -1/3, fdM = (-2/8)/(12/8) = -1/6 (BABA wins:
      the P1 form).
    Window [5, 6): 000011 -> (2, 0, 0): ABBA + BABA = 0, so D is NaN; FD2 += 0, GD1 += 2*(2*2) = 8;
      den = 0: fd and fdM (ABBA >= BABA: the den form) are NaN too.
    Window [5, 7): adds 110100 -> (0, 1, 2): ABBA 2*1*2 = 4; b < c: FD3 += 2*(2*2 - 0) = 8; a < c:
      GD3 += 2*(2*2 - 1*2) = 4.  sums 4, 0, 0, 8, 8, 4: D = 1, fd = fdM = (4/8)/(8/8) = 0.5.
    Window (7, 7) is empty: zeros and NaN."""
    types = np.array(HAND_TYPES, np.uint64)
    flags = np.full(len(types), COUNTED | SEG, np.uint8)
    flags[4] = COUNTED
    masks, pop_n, wins = [0b000011, 0b001100, 0b110000], [2, 2, 2], [(0, 5), (5, 6), (5, 7), (7, 7)]
    sums, d, fd, fdm = ref_dstat(types, flags, masks, pop_n, wins, [(0, 1, 2)])
    assert sums.shape == (4, 1, 6) and sums.dtype == np.int64 and d.shape == fd.shape == fdm.shape == (4, 1)
    assert sums[0, 0].tolist() == [11, 9, 10, 0, 8, 0]
    assert (d[0, 0], fd[0, 0], fdm[0, 0]) == (0.1, 0.25 / 1.25, 0.25 / 1.25)
    assert sums[1, 0].tolist() == [0, 0, 0, 0, 8, 0] and np.isnan([d[1, 0], fd[1, 0], fdm[1, 0]]).all()
    assert sums[2, 0].tolist() == [4, 0, 0, 8, 8, 4] and (d[2, 0], fd[2, 0], fdm[2, 0]) == (1.0, 0.5, 0.5)
    assert not sums[3].any() and np.isnan([d[3, 0], fd[3, 0], fdm[3, 0]]).all()
    # ABBA and BABA are counts of sample triples (x in P1, y in P2, z in P3) with patterns 0,1,1 and 1,0,1
    for outidx in (None, 5):
        s2 = ref_dstat(types, flags, masks, pop_n, wins, [(0, 1, 2)], outidx)[0]
        for w, (beg, end) in enumerate(wins):
            abba = baba = 0
            for r in range(beg, end):
                if not flags[r] & SEG:
                    continue
                t = int(types[r])
                if outidx is not None and (t >> outidx) & 1:
                    t ^= 0b111111   # the derived allele is the other one
                for x, y, z in itertools.product((0, 1), (2, 3), (4, 5)):
                    pat = ((t >> x) & 1, (t >> y) & 1, (t >> z) & 1)
                    abba += pat == (0, 1, 1)
                    baba += pat == (1, 0, 1)
            assert (abba, baba) == (s2[w, 0, 0], s2[w, 0, 1]), (outidx, w)
    # the flip
    s3, d3, fd3, fdm3 = ref_dstat(types, flags, masks, pop_n, wins, [(0, 1, 2)], 5)
    assert s3[0, 0].tolist() == [1, 3, 6, 0, 12, 0]
    assert (d3[0, 0], fd3[0, 0], fdm3[0, 0]) == (-0.5, -0.25 / 0.75, -0.25 / 1.5)
    # a repeated triple and another order are rows of their own
    s4 = ref_dstat(types, flags, masks, pop_n, wins, [(0, 1, 2), (2, 1, 0), (0, 1, 2)])[0]
    assert np.array_equal(s4[:, 0], s4[:, 2]) and np.array_equal(s4[:, 0], sums[:, 0]) and not np.array_equal(s4[:, 0], s4[:, 1])


@pytest.mark.parametrize("outidx", [None, 0, 16])
def test_swapping_p1_and_p2(outidx):
    """(P2, P1, P3) against (P1, P2, P3): ABBA <-> BABA, FD2 <-> GD1, FD3 <-> GD3; D changes sign and
    |fdM| stays (where ABBA != BABA: the two forms trade places with the same numbers; at a tie the
    numerator is zero and the two denominators need not be zero together)."""
    L, sizes = 4000, [5, 7, 6]
    rng = np.random.default_rng(11)
    types = _random_types(rng, L, 18)
    flags = np.where(rng.random(L) < 0.5, COUNTED | SEG, COUNTED).astype(np.uint8)
    wins = [(0, L), (100, 900), (3000, 3003), (7, 8)]
    sums, d, fd, fdm = ref_dstat(types, flags, _blocks(sizes), sizes, wins, [(0, 1, 2), (1, 0, 2), (2, 0, 1), (0, 2, 1)], outidx)
    for x, y in ((0, 1), (2, 3)):
        assert np.array_equal(sums[:, x][:, [1, 0, 4, 5, 2, 3]], sums[:, y])
        ok = ~np.isnan(d[:, x])
        assert ok.sum() >= 2 and np.array_equal(-d[ok, x], d[ok, y]) and np.isnan(d[~ok, y]).all()
        ne = sums[:, x, 0] != sums[:, x, 1]
        fx, fy = fdm[ne, x], fdm[ne, y]
        assert ne.sum() >= 2 and np.where(np.isnan(fx), np.isnan(fy), bits(np.abs(fx)) == bits(np.abs(fy))).all()
        assert np.isfinite(fx).any() and (sums[:, x, 2:] != 0).any(axis=0).all()


def test_dstat_option_parses():
    base = ["-f", "ref.fa", "-w", "10"]
    plain = opt.parse_args("sfs", base + ["in.bam", "chr1:1-500"])
    assert plain.output == 0
    for argv in (base + ["--dstat", "in.bam", "chr1:1-500"], ["--dstat"] + base + ["in.bam", "chr1:1-500"],
                 base + ["in.bam", "--dstat", "chr1:1-500"], base + ["in.bam", "chr1:1-500", "--dstat"]):
        o = opt.parse_args("sfs", argv)
        assert o.output == 4 and (o.bamfile, o.region) == ("in.bam", "chr1:1-500") and o.win_size == plain.win_size
    for extra, want in ((["--theta"], 5), (["--joint"], 6), (["--theta", "--joint"], 7)):
        for argv in (base + extra + ["--dstat", "in.bam", "chr1"], ["--dstat"] + base + ["in.bam", "chr1"] + extra):
            o = opt.parse_args("sfs", argv)
            assert o.output == want and (o.bamfile, o.region) == ("in.bam", "chr1")
    assert opt.parse_args("sfs", base + ["--theta", "--joint", "in.bam", "chr1"]).output == 3
    # only sfs has it
    assert opt.parse_args("nucdiv", base + ["--dstat", "in.bam", "chr1"]).output == 0
    assert opt.parse_args("ld", base + ["--dstat", "in.bam", "chr1"]).output == 0
    # the command line's triples
    assert opt.dstat_triples(4) == [(0, 1, 2), (0, 1, 3), (0, 2, 1), (0, 2, 3), (0, 3, 1), (0, 3, 2),
                                    (1, 2, 0), (1, 2, 3), (1, 3, 0), (1, 3, 2), (2, 3, 0), (2, 3, 1)]
    assert opt.dstat_triples(3) == [(0, 1, 2), (0, 2, 1), (1, 2, 0)] and opt.dstat_triples(2) == [] == opt.dstat_triples(1)
    assert [opt.dstat_triples(k) for k in range(1, 8)] == [all_triples(k) for k in range(1, 8)]
    assert len(opt.dstat_triples(21)) == 3990 <= opt.DSTAT_MAX_TRIPLES == 4096
    with pytest.raises(opt.PopbamError, match="Too many populations for --dstat"):
        opt.dstat_triples(22)


# ---- GPU tests ---------------------------------------------------------------------------
N_SITES = 32_000
SHAPES = [(12, 3), (24, 3), (48, 4), (96, 4), (30, 5)]   # row widths 2 / 4 / 8 / 16 / 4 B; 3, 12 and 30 triples
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
    rng = np.random.default_rng(7)   # tests/test_jsfs.py's ragged layout
    cuts = np.sort(rng.choice(n_sites, 40, replace=False))
    return [(int(a), int(b)) for a, b in zip(cuts[:-1], cuts[1:])] + [(5, 5), (0, 1)]


def _run_dstat(ctx, rows, n_rows, wins, triples, outidx=0):
    from popbam_amd import workload
    j = workload.DStat(ctx, len(wins), triples, outidx)
    j(rows, _wins_tensor(wins), n_rows)
    ctx.sync_check()
    return _arrays(j, NAMES)


def _outgroup(mode, n):
    return {"none": (False, None), "first": (True, 0), "last": (True, n - 1)}[mode]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["none", "first", "last"])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n,npops", SHAPES, ids=SHAPE_IDS)
def test_dstat_matches_the_checker_on_called_rows(gpu_lib, n, npops, layout, mode):
    ctx, ctx_out, params, rows, types, flags = _shape(n, npops)
    wins = _layout(layout, N_SITES)
    masks, pop_n = _pop_masks(params)
    flagged, outidx = _outgroup(mode, n)
    triples = all_triples(npops)
    got = _run_dstat(ctx_out if flagged else ctx, rows, N_SITES, wins, triples, outidx or 0)
    want = ref_dstat(types, flags, masks, pop_n, wins, triples, outidx)
    _assert_same(got, want, (n, npops, layout, mode))
    assert got[0].shape == (len(wins), len(triples), 6)
    assert (got[0][:, :, 0] > 0).any() and (got[0][:, :, 1] > 0).any() and np.isfinite(got[1]).any()
    if mode != "none":   # the flip changed the sums
        plain = ref_dstat(types, flags, masks, pop_n, wins, triples, None)
        assert not np.array_equal(plain[0], got[0])


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


def _topped_up(triples, to):
    return triples + [triples[(7 * k) % len(triples)] for k in range(to - len(triples))]


CRAFTED = {"42+42+42": ([42, 42, 42], list(itertools.permutations((0, 1, 2)))),
           "120+3+3": ([120, 3, 3], list(itertools.permutations((0, 1, 2)))),
           "21pops": ([6] * 21, _topped_up(all_triples(21), 4096))}


@pytest.mark.gpu
@pytest.mark.parametrize("outidx", [None, 125])
@pytest.mark.parametrize("name", list(CRAFTED))
def test_dstat_crafted_rows_of_126_samples(gpu_lib, name, outidx):
    """Every row counted and segregating, random types, n = 126: 42 + 42 + 42 (the largest terms) in
    all six orders of the one triple, 120 + 3 + 3, and 21 populations of 6 with their 3,990 triples
    topped up with repeats to exactly 4,096 -- more than the LDS sums hold, so the triples go in
    groups and the rows are streamed once per group, a lane per triple."""
    sizes, triples = CRAFTED[name]
    L, n = 3000, 126
    assert name != "21pops" or (len(triples) == 4096 and len(set(triples)) == 3990)
    rng = np.random.default_rng(len(sizes))
    types = _random_types(rng, L, n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    masks = _blocks(sizes)
    ctx, params, rows = _crafted(n, masks, types, flags, F_OUTGROUP if outidx is not None else 0)
    wins = [(0, L), (17, 2001), (5, 5), (2999, 3000)]
    got = _run_dstat(ctx, rows, L, wins, triples, outidx or 0)
    _assert_same(got, ref_dstat(types, flags, masks, sizes, wins, triples, outidx), name)
    assert (got[0][0, :, :2] > 0).all() and np.isfinite(got[1][0]).all()
    ctx.close()


@pytest.mark.gpu
def test_dstat_interleaved_masks_and_a_population_of_one(gpu_lib):
    """Samples 0, 2, .. 10, samples 1, 3, .. 11, and sample 12 alone, in all six orders."""
    L, n = 3000, 13
    rng = np.random.default_rng(5)
    types = _random_types(rng, L, n)
    flags = np.where(rng.random(L) < 0.3, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks, sizes = [0b0010101010101, 0b1000000000000, 0b0101010101010], [6, 1, 6]
    triples = list(itertools.permutations((0, 1, 2)))
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (17, 2001)]
    got = _run_dstat(ctx, rows, L, wins, triples)
    _assert_same(got, ref_dstat(types, flags, masks, sizes, wins, triples))
    assert (got[0][:, :, :2] > 0).all() and np.isfinite(got[1]).all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_dstat_partial_last_word(gpu_lib, n, words):
    """Windows that end at n_rows = L = 64 * 5 + 3, no multiple of the rows per 16-byte word; the
    rows sit in a larger buffer of 0xFF bytes, which would read as segregating rows with every
    sample derived.  The same with 513 words and three rows (window_helpers.py): with three
    populations a full queue of 512 rows is two count batches."""
    import torch
    L, more = partial_rows(n, words)
    rng = np.random.default_rng(n)
    types = _random_types(rng, L, n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    sizes = [n // 3, n // 3, n - 2 * (n // 3)]
    masks = _blocks(sizes)
    ctx, params, rows = _crafted(n, masks, types, flags)
    big = torch.full((rows.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:rows.numel()] = rows
    assert words is None or L == words * (16 // ctx.row_bytes) + 3
    wins = [(3, L), (0, L), (L - 1, L)] + more
    triples = all_triples(3)
    got = _run_dstat(ctx, big, L, wins, triples)
    _assert_same(got, ref_dstat(types, flags, masks, sizes, wins, triples))
    assert (got[0][:2, :, :2] > 0).all()
    ctx.close()


@pytest.mark.gpu
def test_dstat_argument_errors(gpu_lib):
    import torch
    from popbam_amd import _lib, workload
    ctx, ctx_out, params, rows, types, flags = _shape(12, 3)
    wins = _wins_tensor([(0, 1000)])
    T = [(0, 1, 2)]
    j = workload.DStat(ctx, 1, T)
    lib, s = ctx.lib, workload.stream_handle()
    r, w, o, out = rows.data_ptr(), wins.data_ptr(), C.byref(j.opts), C.byref(j.out)

    def refused(c, rc):
        assert rc == _lib.PBG_E_ARG
        assert lib.pbg_last_error(c.h)

    assert lib.pbg_window_dstat(None, r, N_SITES, w, 1, o, out, s) == _lib.PBG_E_ARG
    for args in ((None, N_SITES, w, 1, o, out), (r, N_SITES, None, 1, o, out), (r, N_SITES, w, 1, None, out),
                 (r, N_SITES, w, 1, o, None)):
        refused(ctx, lib.pbg_window_dstat(ctx.h, *args, s))
    # the list: its length, a null array, indices, distinct members
    arr = (_lib.PbgTriple * 1)(_lib.PbgTriple(0, 1, 2))
    for nt, ptr in ((-1, arr), (_lib.PBG_DSTAT_MAX_TRIPLES + 1, arr), (1, None)):
        bad = _lib.PbgDstatOpts(0, nt, C.cast(ptr, C.POINTER(_lib.PbgTriple)) if ptr is not None else None)
        refused(ctx, lib.pbg_window_dstat(ctx.h, r, N_SITES, w, 1, C.byref(bad), out, s))
    for t in ((0, 1, 3), (-1, 1, 2), (0, 3, 2), (64, 1, 2), (0, 0, 1), (0, 1, 0), (2, 1, 1), (1, 1, 1)):
        refused(ctx, workload.DStat(ctx, 1, [(0, 1, 2), t]).run(rows, wins, N_SITES))
    for t in itertools.permutations((0, 1, 2)):
        assert workload.DStat(ctx, 1, [t, t]).run(rows, wins, N_SITES) == _lib.PBG_OK
    refused(ctx, workload.DStat(ctx, 1, T * 4097).run(rows, wins, N_SITES))
    full = workload.DStat(ctx, 1, _topped_up(all_triples(3), 4096))
    assert full.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    assert torch.equal(full.sums[0, 0], full.sums[0, 3]) and torch.equal(full.sums[0, 0], full.sums[0, 4095])
    assert full.sums[0, :, 0].min() > 0
    # outidx counts only with the flag: any value without it, a sample index with it
    for outidx in (-1, 12, 1 << 20):
        assert workload.DStat(ctx, 1, T, outidx).run(rows, wins, N_SITES) == _lib.PBG_OK
        refused(ctx_out, workload.DStat(ctx_out, 1, T, outidx).run(rows, wins, N_SITES))
    assert workload.DStat(ctx_out, 1, T, 11).run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    ctx_out.sync_check()
    # no triple: PBG_OK, nothing written
    none = workload.DStat(ctx, 1, [])
    pre = {"sums": torch.full((64,), -7, dtype=torch.int64, device="cuda")}
    for k in NAMES[1:]:
        pre[k] = torch.full((64,), -7.0, dtype=torch.float64, device="cuda")
    none.out = _lib.PbgDstatOut(*(pre[k].data_ptr() for k in NAMES))
    assert none.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    assert all((pre[k] == -7).all() for k in NAMES)
    # a window past the rows is never read: an empty window's outputs, reported by pbg_check
    bad = workload.DStat(ctx, 2, T)
    assert bad.run(rows, _wins_tensor([(0, N_SITES + 1), (0, 1000)]), N_SITES) == _lib.PBG_OK
    assert lib.pbg_check(ctx.h, None) == _lib.PBG_E_RANGE
    assert not bad.sums[0].any() and bad.sums[1, 0, 0] > 0
    assert all(np.isnan(getattr(bad, k)[0].cpu().numpy()).all() for k in NAMES[1:])
    assert j.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    assert torch.equal(j.sums[0], bad.sums[1])


@pytest.mark.gpu
def test_dstat_interleaves_with_the_other_calls(gpu_lib):
    """Statistics, joint spectrum, LD decay, dstat with list A, with list B, with list A again,
    statistics, with the same pointers on one context and stream: each equals its own stand-alone
    run on a fresh context byte for byte; two dstat runs give identical bytes; a NULL member of
    pbg_dstat_out leaves its array untouched and the others correct."""
    from popbam_amd import _lib, workload
    n, npops, L = 12, 3, 64 * 1500
    wins = [(0, L)] + workload.reference_windows(0, L, 10_000)
    A, B = all_triples(3), [(2, 1, 0), (1, 0, 2), (0, 1, 2), (2, 1, 0), (0, 2, 1)]

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

    def same_bytes(got, want, what):
        for g, w_, nm in zip(got, want, what):
            assert g.tobytes() == w_.tobytes(), nm

    JN, DN = ("cells", "diffs", "fst"), ("pairs", "r2_sum", "n_var")
    alone = {}
    for key, make in (("zns", None), ("jsfs", lambda hp: workload.JointSfs.of(hp)),
                      ("decay", lambda hp: workload.LdDecay.of(hp, 100, 100)),
                      ("A", lambda hp: workload.DStat.of(hp, A)), ("B", lambda hp: workload.DStat.of(hp, B))):
        ctx, hp = fresh()
        if make is None:
            zns(hp)
            ctx.sync_check()
            alone[key] = zns_out(hp)
        else:
            x = make(hp)
            ctx.sync_check()
            alone[key] = arrays(x, {"jsfs": JN, "decay": DN}.get(key, NAMES))
        ctx.close()
    assert (alone["A"][0][0, :, :2] > 0).all() and np.isfinite(alone["A"][1][0]).all()
    assert np.array_equal(alone["A"][0][:, 0], alone["B"][0][:, 2]) and not np.array_equal(alone["A"][0][:, 0], alone["B"][0][:, 0])

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    first = zns_out(hp)
    zns(hp)   # a cached plan from here on
    j = workload.JointSfs(ctx, len(wins))
    j(hp.rows, hp.wins, L)
    d = workload.LdDecay(ctx, len(wins), 100, 100)
    d(hp.rows, hp.wins, L)
    da = workload.DStat(ctx, len(wins), A)
    da(hp.rows, hp.wins, L)
    db = workload.DStat(ctx, len(wins), B)
    db(hp.rows, hp.wins, L)
    da2 = workload.DStat(ctx, len(wins), A)
    da2(hp.rows, hp.wins, L)
    zns(hp)
    ctx.sync_check()
    second = zns_out(hp)
    for got in (first, second):
        assert np.array_equal(got[0], alone["zns"][0]) and np.array_equal(got[1], alone["zns"][1])
    same_bytes(arrays(j, JN), alone["jsfs"], JN)
    same_bytes(arrays(d, DN), alone["decay"], DN)
    same_bytes(_arrays(da, NAMES), alone["A"], NAMES)
    same_bytes(_arrays(db, NAMES), alone["B"], NAMES)
    same_bytes(_arrays(da2, NAMES), _arrays(da, NAMES), NAMES)
    for k, drop in enumerate(NAMES):   # a NULL member: the others as before, the dropped array untouched
        part = workload.DStat(ctx, len(wins), A)
        getattr(part, drop).fill_(-3)
        setattr(part.out, drop, None)
        part(hp.rows, hp.wins, L)
        ctx.sync_check()
        got = _arrays(part, NAMES)
        for m, nm in enumerate(NAMES):
            if m == k:
                assert (got[m] == -3).all(), nm
            else:
                assert got[m].tobytes() == alone["A"][m].tobytes(), (drop, nm)
    ctx.close()


@pytest.mark.gpu
def test_dstat_more_lists_than_the_context_keeps(gpu_lib):
    """Twenty lists of different content on one context (it keeps the device copies of 16), each run
    twice, the second round after all of them: every list gives its own triples' sums."""
    from popbam_amd import workload
    ctx, ctx_out, params, rows, types, flags = _shape(12, 3)
    masks, pop_n = _pop_masks(params)
    wins = [(0, 3000), (3000, 3001)]
    perms = list(itertools.permutations((0, 1, 2)))
    want = ref_dstat(types, flags, masks, pop_n, wins, perms)
    lists = [[perms[(k + m) % 6] for m in range(k + 1)] for k in range(20)]
    wt = _wins_tensor(wins)
    for _ in range(2):
        runs = [workload.DStat(ctx, len(wins), tl)(rows, wt, N_SITES) for tl in lists]
        ctx.sync_check()
        for k, (tl, j) in enumerate(zip(lists, runs)):
            idx = [perms.index(t) for t in tl]
            _assert_same(_arrays(j, NAMES), tuple(x[:, idx] for x in want), k)
    assert (want[0][0, :, :2] > 0).all()


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
j = workload.DStat.of(hp, {triples!r})
ctx.sync_check()
np.savez({out!r}, rows=hp.rows.cpu().numpy(), sums=j.sums.cpu().numpy(), d=j.d.cpu().numpy(), fd=j.fd.cpu().numpy(),
         fdm=j.fdm.cpu().numpy())
ctx.close()
print("ok")
"""


@pytest.mark.gpu
def test_dstat_under_the_bounds_build(gpu_lib, tmp_path):
    """The (24, 3) reference-window case through the PBG_BOUNDS build (a fresh process): the same
    rows and the checker's numbers."""
    if not os.path.exists(BOUNDS_LIB):
        pytest.skip("the bounds build is not there (make bounds)")
    n, npops = 24, 3
    ctx, ctx_out, params, rows, types, flags = _shape(n, npops)
    out = str(tmp_path / "bounds.npz")
    env = dict(os.environ, POPBAM_GPU_LIB=BOUNDS_LIB)
    triples = all_triples(npops)
    r = subprocess.run([sys.executable, "-c", BOUNDS_SNIPPET.format(repo=REPO, n=n, npops=npops, n_sites=N_SITES,
                                                                   seed=SEED + n, out=out, triples=triples)],
                       env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    z = np.load(out)
    assert np.array_equal(z["rows"], rows.cpu().numpy())
    masks, pop_n = _pop_masks(params)
    wins = _layout("ref10kb", N_SITES)
    _assert_same(tuple(z[k] for k in NAMES), ref_dstat(types, flags, masks, pop_n, wins, triples), "bounds")


# ---- command lines -----------------------------------------------------------------------
def _split_dstat(ext, pops):
    """The appended --dstat fields of one line -> [(D text, fd text, fdM text, [six sums])] per triple."""
    triples = all_triples(len(pops))
    assert len(ext) == 8 * len(triples), ext[:8]
    out = []
    for t, (i, j, k) in enumerate(triples):
        lab = f"[{pops[i]},{pops[j]},{pops[k]}]:"
        f = ext[8 * t:8 * t + 8]
        assert [f[0], f[2], f[4], f[6]] == ["D" + lab, "fd" + lab, "fdM" + lab, "dsum" + lab], f
        sums = [int(x) for x in f[7].split(",")]
        assert len(sums) == 6
        out.append((f[1], f[3], f[5], sums))
    return out


DSTAT_CASES = [("g03_threepops", 1), ("g15_24s3p", 22), ("g18_64s4p", 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,idx", DSTAT_CASES, ids=[f"{n}-{i:02d}" for n, i in DSTAT_CASES])
def test_dstat_command_line(gpu_lib, name, idx):
    """`popbam sfs --dstat` and `sfs --theta --joint --dstat` through cli.run and the native binary:
    the same text; with the appended columns cut off, the golden text (which is the oracle's); the
    labels and the triple order; dsum[..] holds the checker's integers on the oracle's rows for the
    command; D, fd, fdM are the values recomputed from the printed integers at the printed precision."""
    from popbam_amd import workload
    case = fixtures.load_case(name)
    cs = case["meta"]["cases"][idx]
    argv = _argv(name, cs)
    gold = fixtures.golden_text(name, cs["stdout"]).splitlines()
    st = harness.Setup(name, cs["args"] + ["--dstat"], cs["region"])
    assert st.opts.output == 4
    st.opts.output = 0
    assert harness.oracle_run(st).splitlines() == gold
    _, types, _, flags = harness.oracle_call(st.orc_params(), st.batch)
    outidx = st.outidx if st.opts.flag & opt.BAM_OUTGROUP else None
    assert (outidx is not None) == ("-p" in cs["args"])
    wins = workload.reference_windows(st.beg, st.end, st.opts.win_size)
    pops, npop = st.sm.pops, len(st.sm.pops)
    triples = all_triples(npop)
    want = ref_dstat(types, flags, st.masks, st.pop_n, wins, triples, outidx)[0]
    texts = {}
    for extra in (["--dstat"], ["--theta", "--joint", "--dstat"]):
        ours = cli.run(argv[0], argv[1:] + extra)
        rc, nat, err = _native(argv[:1] + extra + argv[1:])   # the tokens in front here, at the end there
        assert rc == 0, err
        assert nat == ours
        texts[len(extra)] = ours.splitlines()
    assert len(texts[1]) == len(texts[3]) == len(gold) == len(wins) > 0
    finite = 0
    for w, (gl, l1, l3) in enumerate(zip(gold, texts[1], texts[3])):
        assert l1.startswith(gl + "\tD[") and l3.startswith(gl + "\tS["), (gl, l1)
        ext1 = l1[len(gl):].split("\t")[1:]
        ext3 = l3[len(gl):].split("\t")[1:]
        assert ext3[-len(ext1):] == ext1 and ext3[6 * npop].startswith("fst[")   # --theta's, --joint's, then these
        assert len(ext3) == 6 * npop + 4 * (npop * (npop - 1) // 2) + len(ext1)
        for t, (dtxt, fdtxt, fdmtxt, sums) in enumerate(_split_dstat(ext1, pops)):
            assert sums == want[w, t].tolist(), (w, triples[t])
            n1, n2, n3 = (st.pop_n[p] for p in triples[t])
            for txt, v in zip((dtxt, fdtxt, fdmtxt), ratios_of(sums, n1, n2, n3)):
                assert (txt.strip() == "NA") if np.isnan(v) else (txt == "%.5f" % v), (txt, v)
            finite += 0 if dtxt.strip() == "NA" else 1
    assert finite > 0 and want[:, :, :2].sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["g01_base", "g14_onepop"])
def test_dstat_with_fewer_than_three_populations_adds_nothing(gpu_lib, name):
    d = fixtures.load_case(name)["dir"]
    argv = ["sfs", "-f", os.path.join(d, "ref.fa"), "-w", "1", os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run(argv[0], argv[1:])
    assert len(plain.splitlines()) > 0
    if name == "g14_onepop":
        assert plain == open(os.path.join(d, "out", "06_sfs_w1.tsv")).read()
    assert cli.run(argv[0], argv[1:] + ["--dstat"]) == plain
    rc, nat, err = _native(argv + ["--dstat"])
    assert rc == 0 and nat == plain, err
