"""`ld --rmin`: Hudson and Kaplan's Rm, the minimum number of recombination events the four-gamete
test implies, and the intervals that witness them, per window and population (pbg_window_rmin,
include/popbam_gpu.h; DESIGN.md "Rmin").  The reference has no such output, so the checker lives
here: `ref_rmin` restates the header's definition in Python integers -- the columns of the variable
sites, the four-gamete test, L(b) by a double loop and the greedy walk.  Two independent forms check
the checker: an interval DP for the largest number of disjoint incompatible intervals, and the
streaming form the kernel uses (a list of distinct splits that restarts at every cut).  Every
comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import harness
from window_helpers import _arrays, _blocks, mask_words, _native, _wins_tensor
from window_helpers import PARTIAL_WORD_CASES, partial_rows
from popbam_amd import cli
from popbam_amd import options as opt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")
SEED = 0x4A1
COUNTED, SEG = 2, 4   # harness flags bits
NAMES = ("rmin", "n_var", "cuts")


# ---- the checker -----------------------------------------------------------------------
def incompatible(a, b, pm):
    """The four-gamete test on two columns inside population mask pm."""
    return bool(a & b) and bool(a & ~b & pm) and bool(~a & b & pm) and bool(pm & ~(a | b))


def greedy(cols, pm):
    """The definition: L(b) is the largest a < b incompatible with b; an interval is chosen when L(b)
    is at or after the right end of the last chosen one.  -> [(a, b)] as indices into cols."""
    out, c = [], 0
    for b in range(len(cols)):
        left = None
        for a in range(b - 1, -1, -1):   # downwards, so the first hit is the largest
            if incompatible(cols[a], cols[b], pm):
                left = a
                break
        if left is not None and left >= c:
            out.append((left, b))
            c = b
    return out


def dp_disjoint(cols, pm):
    """The largest number of incompatible intervals (a, b) no two of which overlap in more than an end
    site: best[b] over the sites 0 .. b."""
    best = [0] * max(1, len(cols))
    for b in range(1, len(cols)):
        best[b] = best[b - 1]
        for a in range(b):
            if incompatible(cols[a], cols[b], pm):
                best[b] = max(best[b], best[a] + 1)
    return best[-1]


def streaming(cols, pm, n_i):
    """The kernel's form: the distinct splits (a column or its complement) since the last cut, each with
    the last site that showed it.  -> ([(a, b)], the longest list)."""
    out, lst, longest = [], [], 0
    for b, x in enumerate(cols):
        bad = [e for e in lst if incompatible(e[0], x, pm)]
        if bad:
            out.append((max(e[1] for e in bad), b))
            lst = [[x, b]]
        else:
            for e in lst:
                if e[0] == x or e[0] == pm & ~x:
                    e[1] = b
                    break
            else:
                lst.append([x, b])
        longest = max(longest, len(lst))
        assert len(lst) <= max(1, 2 * n_i - 3), (len(lst), n_i)
    return out, longest


def row_ints(types):
    lo, hi = mask_words(types)
    return [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]


def ref_rmin(types, flags, pop_masks, pop_n, wins, min_freq=1, max_cuts=0):
    """rmin[nw, np] i32, n_var[nw, np] i32, cuts[nw, np, max_cuts, 2] i32.  A window with beg >= end, or
    outside the rows, is the empty window."""
    ints = row_ints(types)
    seg = (np.asarray(flags) & SEG) > 0
    L, nw, npop = len(seg), len(wins), len(pop_masks)
    rmin = np.zeros((nw, npop), np.int32)
    n_var = np.zeros((nw, npop), np.int32)
    cuts = np.full((nw, npop, max_cuts, 2), -1, np.int32)
    for w, (beg, end) in enumerate(wins):
        if beg >= end or beg < 0 or end > L:
            continue
        rows = (beg + np.flatnonzero(seg[beg:end])).tolist()
        for i, (pm, n_i) in enumerate(zip(pop_masks, pop_n)):
            site = [(r, ints[r] & pm) for r in rows]
            site = [(r, x) for r, x in site if min_freq <= bin(x).count("1") <= n_i - min_freq]
            chosen = greedy([x for _, x in site], pm)
            rmin[w, i], n_var[w, i] = len(chosen), len(site)
            for k, (a, b) in enumerate(chosen[:max_cuts]):
                cuts[w, i, k] = (site[a][0], site[b][0])
    return rmin, n_var, cuts


def _assert_same(got, want, what=""):
    for g, w, nm in zip(got, want, NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, nm, g.shape, w.shape, g.dtype, w.dtype)
        same = g == w
        assert same.all(), (what, nm, np.argwhere(~same)[:5].tolist(), g[~same][:5], w[~same][:5])


def _tree_splits(rng, n):
    """The clades of a random tree on n leaves (random joining), the leaves included, as bit masks."""
    clusters = [1 << s for s in range(n)]
    splits = list(clusters)
    while len(clusters) > 2:
        a, b = sorted(rng.choice(len(clusters), 2, replace=False).tolist())
        m = clusters[a] | clusters[b]
        del clusters[b], clusters[a]
        clusters.append(m)
        splits.append(m)
    return splits


def _tree_blocks(rng, n, trees, per_tree):
    """Columns that are splits of one tree for a while, randomly complemented, then of another tree."""
    full, cols = (1 << n) - 1, []
    for _ in range(trees):
        sp = _tree_splits(rng, n)
        for _ in range(int(rng.integers(1, per_tree + 1))):
            x = sp[int(rng.integers(0, len(sp)))]
            cols.append(full & ~x if rng.random() < 0.5 else x)
    return [x for x in cols if 0 < x < full]


# ---- CPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 6, 12])
def test_checker_agrees_with_the_interval_dp_and_the_streaming_form(n):
    """Random columns and tree-structured blocks: the greedy count is the DP's maximum, the streaming
    form chooses the same intervals with a list of at most max(1, 2 n - 3) splits, and
    rmin <= max(V - 1, 0)."""
    rng = np.random.default_rng(1000 + n)
    full = (1 << n) - 1
    counts, longest = set(), 0
    for trial in range(600):
        if trial % 2:
            cols = _tree_blocks(rng, n, int(rng.integers(1, 5)), 12)
        else:
            cols = [int(x) for x in rng.integers(1, full, int(rng.integers(0, 25))).tolist()] if n > 1 else []
        g = greedy(cols, full)
        s, ln = streaming(cols, full, n)
        assert g == s, (n, trial, cols)
        assert len(g) == dp_disjoint(cols, full), (n, trial, cols)
        assert len(g) <= max(len(cols) - 1, 0)
        assert all(incompatible(cols[a], cols[b], full) and a < b for a, b in g)
        assert all(g[k][1] <= g[k + 1][0] for k in range(len(g) - 1))
        counts.add(len(g))
        longest = max(longest, ln)
    if n < 4:
        assert counts == {0}   # four gametes need four samples
    else:
        assert len(counts) > 2
    if n == 12:
        assert longest > 8   # the tree blocks grow long lists between cuts


def test_one_tree_never_cuts():
    """All 2 n - 3 splits of a tree, some twice and complemented: no interval, and the list holds them all."""
    rng = np.random.default_rng(5)
    for n in (4, 7, 12):
        full = (1 << n) - 1
        sp = [x for x in _tree_splits(rng, n) if 0 < x < full]
        cols = sp + [full & ~x for x in sp[::2]]
        assert greedy(cols, full) == []
        assert streaming(cols, full, n) == ([], 2 * n - 3)


HAND_TYPES = np.array([0b00110011, 0b00110101, 0b10101010, 0b01110011, 0b00011100, 0b01100001, 0b00000110], np.uint64)
HAND_FLAGS = np.array([COUNTED | SEG, COUNTED | SEG, COUNTED, COUNTED | SEG, COUNTED | SEG, COUNTED | SEG, COUNTED | SEG], np.uint8)
HAND_MASKS, HAND_N = [0b00001111, 0b11110000], [4, 4]
HAND_WINS = [(0, 7), (1, 6), (3, 3)]


def _hand_made_expectations(rmin, n_var, cuts, min_freq, max_cuts):
    """Populations: samples 0..3 and 4..7.  Row 2 is not segregating.  Population 0's columns by row:
      0: 0011   1: 0101   3: 0011   4: 1100   5: 0001   6: 0110
    Row 1 crosses row 0 (gametes 01, 10, 11 and sample 3's 00): interval (0, 1).  Row 3 equals row 0, so
    it crosses row 1, the right end of the last interval: (1, 3), sharing the end site.  Row 4 is row 3's
    complement; it crosses row 1 only, which lies before the last right end: nothing.  Row 5 is a
    singleton.  Row 6 crosses row 4: (4, 6).  Rm = 3.
    Population 1's columns: 0: 0011  1: 0011  3: 0111  4: 0001  5: 0110  6: 0000 (not variable).  Row 5
    crosses rows 0 and 1; the nearer is chosen: (1, 5).  Rm = 1.
    Window [1, 6) drops rows 0 and 6: (1, 3) | (1, 5).  Window (3, 3) is empty."""
    assert rmin.tolist() == [[3, 1], [1, 1], [0, 0]]
    assert n_var.tolist() == ([[6, 5], [4, 4], [0, 0]] if min_freq == 1 else [[5, 3], [3, 2], [0, 0]])
    want = [[[(0, 1), (1, 3), (4, 6)], [(1, 5)]], [[(1, 3)], [(1, 5)]], [[], []]]
    for w in range(3):
        for i in range(2):
            full = (want[w][i] + [(-1, -1)] * max_cuts)[:max_cuts]
            assert [tuple(x) for x in cuts[w, i].tolist()] == full, (w, i)


@pytest.mark.parametrize("min_freq", [1, 2])
def test_checker_on_a_hand_made_window(min_freq):
    for max_cuts in (0, 2, 4):
        got = ref_rmin(HAND_TYPES, HAND_FLAGS, HAND_MASKS, HAND_N, HAND_WINS, min_freq, max_cuts)
        _hand_made_expectations(*got, min_freq, max_cuts)


def test_rmin_option_parses():
    base = ["-f", "ref.fa", "-w", "10"]
    for o_args, want in (([], 0), (["-o", "1"], 1), (["-o", "2"], 2), (["-e"], 0), (["--decay=5,5"], 0)):
        plain = opt.parse_args("ld", base + o_args + ["in.bam", "chr1:1-500"])
        assert (plain.rmin, plain.output) == (0, want)
        for argv in (base + o_args + ["--rmin", "in.bam", "chr1:1-500"], ["--rmin"] + base + o_args + ["in.bam", "chr1:1-500"],
                     base + o_args + ["in.bam", "--rmin", "chr1:1-500"], base + o_args + ["in.bam", "chr1:1-500", "--rmin"]):
            o = opt.parse_args("ld", argv)
            assert o.rmin == 1
            o.rmin = 0
            assert o == plain   # every other field as without the token
    # only ld has it
    for cmd in ("nucdiv", "sfs", "haplo", "diverge", "snp", "tree"):
        assert opt.parse_args(cmd, base + ["--rmin", "in.bam", "chr1"]).rmin == 0
    with pytest.raises(opt.PopbamError, match="Not a valid output option"):
        opt.parse_args("ld", base + ["-o", "3", "--rmin", "in.bam", "chr1"])


def test_native_rmin_errors_match_the_python_cli(capsys):
    d = fixtures.load_case("g01_base")["dir"]
    ref, bam = os.path.join(d, "ref.fa"), os.path.join(d, "in.bam")
    want = {"-o 3 --rmin": "Not a valid output option", "--rmin -o 1 --decay=5,5": "--decay needs -o 0",
            "--rmin --decay=0,5": "Not a valid decay option"}
    for extra, msg in want.items():
        argv = ["ld", "-f", ref] + extra.split() + [bam, "chr1"]
        rc, out, err = _native(argv)
        prc = cli.main(argv)
        pe = capsys.readouterr()
        assert rc == prc == 1 and out == "" == pe.out, argv
        assert err == pe.err and msg in err, (argv, err, pe.err)


def test_rmin_is_exported():
    from popbam_amd import _lib, workload
    assert "pbg_window_rmin" in _lib.EXPORTS and hasattr(workload, "Rmin")
    # a bit of pbg_cmd.output, no new field: a program compiled against the header before it keeps running
    assert _lib.PBG_LD_RMIN == 4 and ("hfs", C.c_int32) == _lib.PbgCmd._fields_[-1]


# ---- GPU tests ---------------------------------------------------------------------------
N_SITES = 32_000
SHAPES = {   # name -> (samples, population masks): the shapes of test_hfs.py
    "n12p2": (12, _blocks([6, 6])),                                   # 2-byte rows
    "n24p3": (24, _blocks([8, 8, 8])),                                # 4-byte rows
    "n40p2i": (40, [sum(1 << s for s in range(0, 40, 2)), sum(1 << s for s in range(1, 40, 2))]),   # 8-byte rows
    "n96p4": (96, _blocks([24] * 4)),                                 # 16-byte rows
    "n126p3": (126, _blocks([70, 50, 6])),                            # population 0 straddles the words, two entries per lane
    "n14one": (14, [0b00000000111111, 0b00000001000000, 0b11111100000000]),   # a population of one; sample 7 in none
}
_shapes = {}


def _params(n, masks, flag=0):
    from popbam_amd import workload
    params = workload.default_params(n, len(masks), flag=flag)
    for i, m in enumerate(masks):
        params.set_pop_mask(i, m)
        params.pop_n[i] = bin(m).count("1")
    return params


def _shape(name):
    """One called synthetic batch per shape, shared by the tests (read only)."""
    if name not in _shapes:
        import torch
        from popbam_amd import _lib, workload
        n, masks = SHAPES[name]
        params = _params(n, masks)
        ctx = _lib.Context(params, 0)
        syn = workload.SynthPileup(ctx, N_SITES, 10, SEED + n)
        hp = workload.HotPath(ctx, syn, [(0, N_SITES)], _lib.PBG_S_SFS)
        hp.call()
        ctx.sync_check()
        torch.cuda.synchronize()
        types, flags = harness.rows_to_sites(hp.rows.cpu().numpy(), ctx.row_bytes, N_SITES, n)
        _shapes[name] = (ctx, params, hp.rows, types, flags)
    return _shapes[name]


def _windows(n_sites):
    """Windows from 3 rows to the whole batch: overlapping, empty, beg == end."""
    rng = np.random.default_rng(7)
    wins = [(0, n_sites), (0, 10_000), (9_999, 20_001), (5, 5), (0, 1), (9, 4)]
    for ln in (3, 10, 30, 60, 100, 150, 300, 1000, 3000):
        for s in rng.integers(0, n_sites - ln, 3):
            wins.append((int(s), int(s) + ln))
    return wins


def _run_rmin(ctx, rows, n_rows, wins, min_freq=1, max_cuts=0):
    from popbam_amd import workload
    j = workload.Rmin(ctx, len(wins), min_freq, max_cuts)
    j(rows, _wins_tensor(wins), n_rows)
    ctx.sync_check()
    return _arrays(j, NAMES)


def _run_with_cuts(ctx, rows, n_rows, wins, min_freq=1):
    """The way the command line sizes the intervals: the counts first, then max_cuts = the largest."""
    rmin, n_var, none = _run_rmin(ctx, rows, n_rows, wins, min_freq, 0)
    assert none.shape == (len(wins), rmin.shape[1], 0, 2)
    mc = int(rmin.max())
    if mc == 0:
        return (rmin, n_var, none), 0
    got = _run_rmin(ctx, rows, n_rows, wins, min_freq, mc)
    assert np.array_equal(got[0], rmin) and np.array_equal(got[1], n_var)
    return got, mc


def _check_against_ref(ctx, rows, types, flags, masks, wins, what=""):
    """Both min_freq values against the checker; rmin and cuts agree between them; the identities."""
    pop_n = [bin(m).count("1") for m in masks]
    res = {}
    for mf in (1, 2):
        got, mc = _run_with_cuts(ctx, rows, len(flags), wins, mf)
        _assert_same(got, ref_rmin(types, flags, masks, pop_n, wins, mf, mc), (what, mf))
        assert (got[0] <= np.maximum(got[1] - 1, 0)).all()
        res[mf] = got
    assert np.array_equal(res[1][0], res[2][0]) and np.array_equal(res[1][2], res[2][2])
    assert (res[1][1] >= res[2][1]).all()
    return res[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_rmin_matches_the_checker_on_called_rows(gpu_lib, name):
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    wins = _windows(N_SITES)
    rmin, n_var, cuts = _check_against_ref(ctx, rows, types, flags, masks, wins, name)
    assert rmin.max() > 0 and n_var.max() > 1
    assert not rmin[3:6].any() and not n_var[[3, 5]].any() and (cuts[3:6] == -1).all()
    if name == "n14one":
        assert not rmin[:, 1].any() and n_var[:, 1].max() == 0   # one sample: no variable site at all


def _founder_types(rng, L, n, founders):
    """Rows in which every sample copies one of a few founders (the copy changes every 64 rows): the
    columns of a stretch are unions of founder groups, so incompatibilities are rare and lists grow."""
    out = np.zeros((L, 2), np.uint64)
    for r0 in range(0, L, 64):
        src = rng.integers(0, founders, n)
        fb = rng.integers(0, 2, (min(64, L - r0), founders))
        sb = fb[:, src]   # [rows, n]
        for s in range(n):
            out[r0:r0 + len(sb), s >> 6] |= sb[:, s].astype(np.uint64) << np.uint64(s & 63)
    return out if n > 64 else out[:, 0].copy()


def _crafted(n, masks, types, flags):
    """A context with the given population masks and device rows packed from (types, flags)."""
    import torch
    from popbam_amd import _lib
    params = _params(n, masks)
    ctx = _lib.Context(params, 0)
    rows = torch.from_numpy(harness.rows_from_oracle(types, flags, ctx.row_bytes).copy()).cuda()
    return ctx, params, rows


def _padded(rows):
    """The rows in a larger buffer of 0xFF bytes."""
    import torch
    big = torch.full((rows.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:rows.numel()] = rows
    return big


FOUNDER = [(12, 3, [6, 6]), (40, 4, [20, 20]), (96, 5, [48, 24, 24])]   # (samples, founders, population sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("n,founders,sizes", FOUNDER, ids=[f"n{a}" for a, _, _ in FOUNDER])
def test_rmin_on_founder_rows(gpu_lib, n, founders, sizes):
    L = 6000
    rng = np.random.default_rng(200 + n)
    types = _founder_types(rng, L, n, founders)
    flags = np.where(rng.random(L) < 0.3, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = _blocks(sizes)
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (0, 64), (64, 128), (30, 100), (100, 612), (1000, 3100), (5990, L), (7, 8)]
    rmin, n_var, cuts = _check_against_ref(ctx, rows, types, flags, masks, wins, n)
    assert rmin[0].min() > 0 and n_var[0].min() > 100
    # a stretch of 64 rows with three founders holds three distinct haplotypes: no four gametes
    assert founders > 3 or (not rmin[1:3].any() and n_var[1:3].min() > 2)
    ctx.close()


def _caterpillar_rows(n, rng):
    """The 2 n - 3 splits of the caterpillar tree on leaves 0 .. n-1 (the n leaves and the prefixes
    {0 .. k}, k = 1 .. n-3) in random order; then 40 of them again, every other one complemented, so the
    last row of a split moves; then {1, n-2}, which crosses every prefix; rows that are not segregating in
    between.  -> (types, flags, the crossing row)."""
    full = (1 << n) - 1
    splits = [1 << s for s in range(n)] + [(1 << (k + 1)) - 1 for k in range(1, n - 2)]
    assert len(splits) == 2 * n - 3
    order = [splits[j] for j in rng.permutation(len(splits))]
    again = [splits[j] for j in rng.integers(0, len(splits), 40)]
    cols = order + [full & ~x if k % 2 else x for k, x in enumerate(again)] + [(1 << 1) | (1 << (n - 2))]
    ints, flags = [], []
    for x in cols:
        if rng.random() < 0.3:   # a row without the segregating bit, with bits that would cross
            ints.append(int(rng.integers(1, 1 << 12)) * 5 & full)
            flags.append(COUNTED)
        ints.append(x)
        flags.append(COUNTED | SEG)
    types = np.array([[x & ((1 << 64) - 1), x >> 64] for x in ints], np.uint64)
    return (types if n > 64 else types[:, 0].copy()), np.array(flags, np.uint8), len(ints) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("n", [12, 126])
def test_rmin_caterpillar_fills_the_list_then_one_site_crosses(gpu_lib, n):
    """Crafted rows (a): every split of one tree is in the list (n - 3 entries that are no leaves, 123 at
    126 samples: two per lane, two-word masks) when the crossing site arrives; Rm = 1 and the left end is
    the last row that showed a prefix or its complement."""
    rng = np.random.default_rng(n)
    types, flags, cross = _caterpillar_rows(n, rng)
    L = len(flags)
    full = (1 << n) - 1
    ctx, params, rows = _crafted(n, [full], types, flags)
    wins = [(0, L), (0, L - 1), (3, L)]
    rmin, n_var, cuts = _check_against_ref(ctx, rows, types, flags, [full], wins, n)
    cols = [x for x, f in zip(row_ints(types), flags.tolist()) if f & SEG]
    assert streaming(cols, full, n)[1] == 2 * n - 3
    assert rmin[:, 0].tolist() == [1, 0, 1] and n_var[0, 0] == len(cols)
    assert cuts[0, 0, 0, 1] == cross and 0 <= cuts[0, 0, 0, 0] < cross
    ctx.close()


def _crafted_rows():
    """14 samples (2-byte rows: 512 rows per trip of the stream, 2,048 per group of loads): population 0
    = samples 0..7, then populations of 1, 2 and 3 samples.  Rows are counted and not segregating unless
    set here; the small populations get random bits in every set row."""
    L = 4200
    rng = np.random.default_rng(14)
    types = np.zeros(L, np.uint64)
    flags = np.full(L, COUNTED, np.uint8)
    A, B = 0b00000011, 0b00000101

    def seg(r, t):
        types[r], flags[r] = np.uint64(t | (int(rng.integers(0, 64)) << 8)), COUNTED | SEG

    # (b) A, B, A, B, ...: every site crosses the one before it
    alt = list(range(5, 3005, 2)) + list(range(3005, 3105))
    for k, r in enumerate(alt):
        seg(r, A if k % 2 == 0 else B)
    # (c) P .. A .. B .. Q: P and Q cross each other and neither A nor B; A and B cross
    far = {"P": 3300, "A": 3310, "B": 3311, "Q": 3400}
    seg(far["P"], A << 4)
    seg(far["A"], A)
    seg(far["B"], B)
    seg(far["Q"], B << 4)
    # the same without the near pair: the far one is found
    seg(3500, A << 4)
    seg(3600, B << 4)
    return types, flags, alt, far


@pytest.mark.gpu
def test_rmin_crafted_rows(gpu_lib):
    """Crafted rows (b) to (e)."""
    types, flags, alt, far = _crafted_rows()
    masks = _blocks([8, 1, 2, 3])
    ctx, params, rows = _crafted(14, masks, types, flags)
    L = len(flags)
    wins = [(0, 3105), (alt[0], alt[-1] + 1), (511, 515), (3200, 3450), (3450, 3700), (0, L)]
    rmin, n_var, cuts = _check_against_ref(ctx, rows, types, flags, masks, wins)
    # (b) Rm = V - 1, the intervals share their end sites
    V = len(alt)
    for w in (0, 1):
        assert rmin[w, 0] == V - 1 == n_var[w, 0] - 1
        assert cuts[w, 0, :V - 1, 0].tolist() == alt[:-1] and cuts[w, 0, :V - 1, 1].tolist() == alt[1:]
    assert rmin[2, 0] == 1 and cuts[2, 0, 0].tolist() == [511, 513]
    # (c) the near pair is chosen, and the far one when there is no near one
    assert rmin[3, 0] == 1 and cuts[3, 0, 0].tolist() == [far["A"], far["B"]] and (cuts[3, 0, 1:] == -1).all()
    assert rmin[4, 0] == 1 and cuts[4, 0, 0].tolist() == [3500, 3600]
    # the whole batch: the last B, then A, B of (c); Q crosses P before the last right end; then two more
    assert rmin[5, 0] == V - 1 + 4 and cuts[5, 0, V - 1:V + 3].tolist() == [[alt[-1], 3310], [3310, 3311], [3400, 3500], [3500, 3600]]
    # (d) populations of 1, 2 and 3 samples
    assert not rmin[:, 1:].any() and (cuts[:, 1:] == -1).all()
    assert n_var[5, 1] == 0 and n_var[5, 2] > 10 and n_var[5, 3] > 10
    # (e) max_cuts below rmin: the first intervals, then -1, and the full count
    for mc in (1, 3, 70):
        r3, v3, c3 = _run_rmin(ctx, rows, L, wins, 1, mc)
        assert np.array_equal(r3, rmin) and np.array_equal(v3, n_var)
        assert np.array_equal(c3, cuts[:, :, :mc]) and (c3[0, 0] >= 0).all() and (c3[3, 0, 1:] == -1).all()
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_rmin_partial_last_word(gpu_lib, n, words):
    """Windows that end at n_rows = L, no multiple of the rows per 16-byte word; the rows sit in a larger
    buffer of 0xFF bytes, which would read as segregating rows with every sample set.  Every row is
    segregating and the columns alternate between two crossing patterns (now and then a complement or
    a leaf), so intervals end on the last row of a trip and start on the first of the next
    (window_helpers.py)."""
    L, more = partial_rows(n, words)
    rng = np.random.default_rng(n)
    sizes = [n // 3, n // 3, n - 2 * (n // 3)]
    masks = _blocks(sizes)
    ints = [0] * L
    for i, (pm, sz) in enumerate(zip(masks, sizes)):
        lo = (pm & -pm).bit_length() - 1
        pat = [0b0011 << lo, 0b0101 << lo, pm & ~(0b0011 << lo), 1 << (lo + sz - 1)]
        pick = np.where(rng.random(L) < 0.15, rng.integers(2, 4, L), (np.arange(L) + i) % 2)
        for a, b in [(0, 2), (L - 2, L)] + more:   # these rows alternate for certain
            pick[a:b] = (np.arange(a, b) + i) % 2
        for r in range(L):
            ints[r] |= pat[int(pick[r])]
    types = np.array([[x & ((1 << 64) - 1), x >> 64] for x in ints], np.uint64)
    types = types if n > 64 else types[:, 0].copy()
    flags = np.full(L, COUNTED | SEG, np.uint8)
    ctx, params, rows = _crafted(n, masks, types, flags)
    big = _padded(rows)
    assert words is None or L == words * (16 // ctx.row_bytes) + 3
    wins = [(3, L), (0, L), (L - 1, L), (L - 9, L), (1, 2), (L - 2, L)] + more
    rmin, n_var, cuts = _check_against_ref(ctx, big, types, flags, masks, wins, (n, words))
    assert (rmin[:2] > L // 4).all() and (n_var[0] == L - 3).all() and (rmin[3] > 0).all()
    assert (cuts[1, :, 0] == np.array([0, 1])).all()   # the batch's first two rows cross
    assert (cuts[1].max(axis=(1, 2)) == L - 1).all()   # an interval ends on the batch's last row
    if more:   # the last row of one trip and the first of the next
        assert (rmin[len(wins) - 1] == 1).all()
    ctx.close()


@pytest.mark.gpu
def test_rmin_argument_errors(gpu_lib):
    from popbam_amd import _lib, workload
    ctx, params, rows, types, flags = _shape("n12p2")
    wins = _wins_tensor([(0, 1000)])
    j = workload.Rmin(ctx, 1, 1, 8)
    lib, s = ctx.lib, workload.stream_handle()
    r, w, o, out = rows.data_ptr(), wins.data_ptr(), C.byref(j.opts), C.byref(j.out)
    assert lib.pbg_window_rmin(None, r, N_SITES, w, 1, o, out, s) == _lib.PBG_E_ARG
    for args in ((None, N_SITES, w, 1, o, out), (r, N_SITES, None, 1, o, out), (r, N_SITES, w, 1, None, out),
                 (r, N_SITES, w, 1, o, None)):
        assert lib.pbg_window_rmin(ctx.h, *args, s) == _lib.PBG_E_ARG
        assert lib.pbg_last_error(ctx.h)
    for mf, mc, msg in ((0, 8, b"min_freq"), (3, 8, b"min_freq"), (1, -1, b"max_cuts"), (1, 0, b"max_cuts")):
        bad = _lib.PbgRminOpts(mf, mc)   # the last: cuts wanted with no room for one
        assert lib.pbg_window_rmin(ctx.h, r, N_SITES, w, 1, C.byref(bad), out, s) == _lib.PBG_E_ARG
        assert msg in lib.pbg_last_error(ctx.h)
    # no cuts array: max_cuts == 0 is fine, and so is max_cuts > 0
    for mc in (0, 5):
        none = _lib.PbgRminOut(j.rmin.data_ptr(), j.n_var.data_ptr(), None)
        assert lib.pbg_window_rmin(ctx.h, r, N_SITES, w, 1, C.byref(_lib.PbgRminOpts(1, mc)), C.byref(none), s) == _lib.PBG_OK
    # no window: PBG_OK, nothing written
    assert workload.Rmin(ctx, 0, 1, 8).run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    # a window past the rows is never read: an empty window's outputs, reported by pbg_check
    over = workload.Rmin(ctx, 3, 1, 8)
    for t in (over.rmin, over.n_var, over.cuts):
        t.fill_(7)
    assert over.run(rows, _wins_tensor([(0, N_SITES + 1), (0, 1000), (-1, 10)]), N_SITES) == _lib.PBG_OK
    assert lib.pbg_check(ctx.h, None) == _lib.PBG_E_RANGE
    assert j.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    for w_ in (0, 2):
        assert not over.rmin[w_].any() and not over.n_var[w_].any() and (over.cuts[w_] == -1).all()
    for nm in NAMES:
        assert getattr(over, nm)[1].cpu().numpy().tobytes() == getattr(j, nm)[0].cpu().numpy().tobytes(), nm
    assert j.rmin[0].min() > 0


@pytest.mark.gpu
def test_rmin_interleaves_with_the_other_calls(gpu_lib):
    """Statistics, decay, Rmin, joint spectrum, Rmin, D statistics, the haplotype spectrum, Rmin,
    statistics, with the same pointers on one context and stream: each equals its own stand-alone run on
    a fresh context byte for byte; a NULL member of pbg_rmin_out leaves its array untouched."""
    from popbam_amd import _lib, workload
    n, npops, L = 12, 3, 64 * 500
    wins = [(0, L)] + workload.reference_windows(0, L, 10_000) + [(s, s + 400) for s in range(0, 8000, 200)]
    T = [(0, 1, 2), (0, 2, 1), (1, 2, 0)]
    MC = 16

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
        return hp.out.t["ld_snps"].cpu().numpy().tobytes(), hp.out.t["ld_val"].cpu().numpy().tobytes()

    def same_bytes(got, want, what):
        for g, w_, nm in zip(got, want, what):
            assert g.tobytes() == w_.tobytes(), nm

    names_of = {"jsfs": ("cells", "diffs", "fst"), "decay": ("pairs", "r2_sum", "n_var"), "dstat": ("sums", "d", "fd", "fdm"),
                "hfs": workload.Hfs.NAMES, "rmin": NAMES}
    make = {"jsfs": lambda ctx: workload.JointSfs(ctx, len(wins)), "decay": lambda ctx: workload.LdDecay(ctx, len(wins), 100, 100),
            "dstat": lambda ctx: workload.DStat(ctx, len(wins), T), "hfs": lambda ctx: workload.Hfs(ctx, len(wins)),
            "rmin": lambda ctx: workload.Rmin(ctx, len(wins), 1, MC)}
    alone = {}
    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    alone["zns"] = zns_out(hp)
    ctx.close()
    for key in make:
        ctx, hp = fresh()
        x = make[key](ctx)(hp.rows, hp.wins, L)
        ctx.sync_check()
        alone[key] = _arrays(x, names_of[key])
        ctx.close()
    assert alone["rmin"][0].max() > 0

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    first = zns_out(hp)
    order = ("decay", "rmin", "jsfs", "rmin", "dstat", "hfs", "rmin")
    ran = []
    for key in order:
        ran.append((key, make[key](ctx)(hp.rows, hp.wins, L)))
    zns(hp)
    ctx.sync_check()
    assert first == alone["zns"] == zns_out(hp)
    for key, x in ran:
        same_bytes(_arrays(x, names_of[key]), alone[key], names_of[key])
    for k, drop in enumerate(NAMES):   # a NULL member: the others as before, the dropped array untouched
        part = workload.Rmin(ctx, len(wins), 1, MC)
        getattr(part, drop).fill_(3)
        setattr(part.out, drop, None)
        part(hp.rows, hp.wins, L)
        ctx.sync_check()
        got = _arrays(part, NAMES)
        for m, nm in enumerate(NAMES):
            if m == k:
                assert (got[m] == 3).all(), nm
            else:
                assert got[m].tobytes() == alone["rmin"][m].tobytes(), (drop, nm)
    ctx.close()


BOUNDS_SNIPPET = r"""
import sys, numpy as np, torch
sys.path.insert(0, {repo!r}); sys.path.insert(0, {repo!r} + "/tests")
from popbam_amd import _lib, workload
assert _lib.load().pbg_build_info() == b"bounds"
params = workload.default_params({n}, {npops})
for i, m in enumerate({masks!r}):
    params.set_pop_mask(i, m)
    params.pop_n[i] = bin(m).count("1")
ctx = _lib.Context(params, 0)
syn = workload.SynthPileup(ctx, {n_sites}, 10, {seed})
hp = workload.HotPath(ctx, syn, {wins!r}, _lib.PBG_S_SFS)
hp.call()
ctx.sync_check()
j = workload.Rmin.of(hp, 1, {max_cuts})
ctx.sync_check()
np.savez({out!r}, rows=hp.rows.cpu().numpy(), **{{k: getattr(j, k).cpu().numpy() for k in workload.Rmin.NAMES}})
ctx.close()
print("ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12p2", "n40p2i", "n126p3"])
def test_rmin_under_the_bounds_build(gpu_lib, tmp_path, name):
    """Called rows through the PBG_BOUNDS build (a fresh process): the same rows and the checker's numbers."""
    if not os.path.exists(BOUNDS_LIB):
        pytest.skip("the bounds build is not there (make bounds)")
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    out = str(tmp_path / "bounds.npz")
    env = dict(os.environ, POPBAM_GPU_LIB=BOUNDS_LIB)
    wins = _windows(N_SITES)
    mc = 24
    r = subprocess.run([sys.executable, "-c", BOUNDS_SNIPPET.format(repo=REPO, n=n, npops=len(masks), masks=masks, n_sites=N_SITES,
                                                                   seed=SEED + n, out=out, wins=wins, max_cuts=mc)],
                       env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    z = np.load(out)
    assert np.array_equal(z["rows"], rows.cpu().numpy())
    pop_n = [bin(m).count("1") for m in masks]
    _assert_same(tuple(z[k] for k in NAMES), ref_rmin(types, flags, masks, pop_n, wins, 1, mc), "bounds")


# ---- command lines -----------------------------------------------------------------------
def _split_rmin(line, pops):
    """(the part before the Rmin columns, {pop: (count, [(left, right)])})."""
    at = line.index("\tRmin[")
    f = line[at + 1:].split("\t")
    assert len(f) == 4 * len(pops), f
    ext = {}
    for i, p in enumerate(pops):
        a, cnt, b, lst = f[4 * i:4 * i + 4]
        assert (a, b) == (f"Rmin[{p}]:", f"rint[{p}]:"), f
        ext[p] = (int(cnt), [] if lst == "NA" else [tuple(int(v) for v in x.split("-")) for x in lst.split(",")])
    return line[:at], ext


CMD_CASES = [(nm, extra) for nm in ("g01_base", "g02_interleaved", "g03_threepops", "g15_24s3p")
             for extra in ((), ("-o", "1"), ("-o", "2"))] + [("g01_base", ("--decay=50,20",)), ("g03_threepops", ("-e",))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", CMD_CASES, ids=[nm + "".join(e).replace("-", "") for nm, e in CMD_CASES])
def test_rmin_command_line(gpu_lib, name, extra):
    """`popbam ld -w 1 [-o N | --decay=50,20 | -e] --rmin` through cli.run and the native binary: the same
    text from both; the part before the Rmin columns is the run without --rmin (the golden text where
    there is one); the appended fields hold the library's numbers for the stream's rows, which are the
    checker's on those rows; the positions lie inside the window's printed range."""
    import torch
    from popbam_amd import _lib, engine, workload
    case = fixtures.load_case(name)
    d = case["dir"]
    args = ["ld", "-w", "1"] + list(extra)
    base = ["ld", "-f", os.path.join(d, "ref.fa"), "-w", "1"] + list(extra)
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run(base[0], base[1:] + tail)
    ours = cli.run(base[0], base[1:] + ["--rmin"] + tail)
    rc, nat, err = _native(base[:1] + ["--rmin"] + base[1:] + tail)   # the token in front here, at the end there
    assert rc == 0, err
    assert nat == ours
    gold = [c for c in case["meta"]["cases"] if c["args"] == args]
    if gold:
        assert plain == fixtures.golden_text(name, gold[0]["stdout"])
    else:
        assert extra == ("--decay=50,20",)
    # the library on the stream's rows and the command's windows
    st = harness.Setup(name, args + ["--rmin"], "chr1")
    assert st.opts.rmin == 1 and st.opts.min_freq == (2 if "-e" in extra else 1)
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
    (rmin, n_var, cuts), mc = _run_with_cuts(ctx, rows, L, wins, st.opts.min_freq)
    types, flags = harness.rows_to_sites(rows.cpu().numpy(), ctx.row_bytes, L, st.sm.n)
    _assert_same((rmin, n_var, cuts), ref_rmin(types, flags, st.masks, st.pop_n, wins, st.opts.min_freq, mc), name)
    lines, plain_lines = ours.splitlines(), plain.splitlines()
    assert len(lines) == len(plain_lines) == len(wins) > 0
    for w, (line, pl) in enumerate(zip(lines, plain_lines)):
        head, ext = _split_rmin(line, st.sm.pops)
        assert head == pl
        f = head.split("\t")
        lo, hi = int(f[1]), int(f[2])
        for i, p in enumerate(st.sm.pops):
            cnt, ivs = ext[p]
            assert cnt == rmin[w, i] == len(ivs)
            assert ivs == [(a + 1, b + 1) for a, b in cuts[w, i, :cnt].tolist()]   # rows are contig positions here
            assert all(lo <= a < b <= hi for a, b in ivs)
    ctx.close()
