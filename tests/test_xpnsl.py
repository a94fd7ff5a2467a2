"""`haplo --xpnsl`: the cross-population nSL tract sums (XP-nSL, Szpiech et al. 2021) per window and
population pair (pbg_window_xpnsl, include/popbam_gpu.h; DESIGN.md "XP-nSL").  The reference has no such
output, so the checker lives here.  `chain_scalar` restates the header's definition literally: per pooled
site, side and sample pair, expand left and right while the pair agrees.  `chain_sums` is the same
expansion with a side's pairs at a site held as the bits of one Python integer, so that a window of
thousands of sites stays within a second; `ref_xpnsl` lays its numbers out as the call does.  An
independent form (`chain_runs`: every pair's agreement sequence cut into maximal runs, each run's length
credited to its sites) checks both.  Every comparison is exact; the printed value is compared as the %.5f
of Python's math.log of the same two divisions."""
import ctypes as C
import math
import os
from functools import partial

import numpy as np
import pytest

import fixtures
import harness
import tract_helpers
from tract_helpers import BOUNDS_LIB, COUNTED, NAMES, N_SITES, SEED, SEG, SHAPES, WIDE
from tract_helpers import local_bits, row_ints, _assert_same, _founder_cols, _params, _shape, _windows, _run_nsl, _run_xpnsl
from tract_helpers import _founder_types, _crafted, _padded, _interleaving, _bounds_child
from window_helpers import _arrays, _blocks, _native, _wins_tensor
from window_helpers import PARTIAL_WORD_CASES, partial_rows
from popbam_amd import cli
from popbam_amd import options as opt

_run_sized = partial(tract_helpers._run_sized, run=_run_xpnsl)


# ---- the checker -----------------------------------------------------------------------
def pairs_of(np_):
    """Population pairs (i, j), i < j, in lexicographic order."""
    return [(i, j) for i in range(np_) for j in range(i + 1, np_)]


def chain_scalar(cols):
    """The definition for one side.  cols[k]: the side's bits at pooled site k.  -> per site (sl, cens)."""
    V = len(cols)
    out = []
    for k in range(V):
        n = len(cols[k])
        sl = cens = 0
        for u in range(n):
            for v in range(u + 1, n):
                if cols[k][u] != cols[k][v]:
                    continue
                l = 1
                while k - l >= 0 and cols[k - l][u] == cols[k - l][v]:
                    l += 1
                r = 1
                while k + r < V and cols[k + r][u] == cols[k + r][v]:
                    r += 1
                sl += l + r - 1
                cens += (l == k + 1) + (r == V - k)
        out.append((sl, cens))
    return out


def _agree_sets(cols):
    """Per site the side's agreeing pairs as the bits of one integer (pair (u, v), u < v, row-major)."""
    if not cols or len(cols[0]) < 2:
        return [0] * len(cols)
    b = np.array(cols, dtype=bool)
    iu, iv = np.triu_indices(b.shape[1], 1)
    packed = np.packbits(b[:, iu] == b[:, iv], axis=1)
    return [int.from_bytes(r.tobytes(), "big") for r in packed]


def chain_sums(cols):
    """chain_scalar with a site's pairs as one integer: the pairs agreeing at k are expanded to the left
    and to the right while any of them still agrees; each step adds the survivors' count."""
    agree = _agree_sets(cols)
    V = len(agree)
    out = []
    for k in range(V):
        sl = cens = 0
        for step in (-1, 1):
            alive, j = agree[k], k
            while alive:
                sl += alive.bit_count()
                j += step
                if j < 0 or j >= V:
                    cens += alive.bit_count()   # the run reaches the window's first / last pooled site
                    break
                alive &= agree[j]
        out.append((sl - agree[k].bit_count(), cens))   # L = l + r - 1
    return out


def chain_runs(cols):
    """The independent form: every pair's agreement sequence cut into maximal runs; a run of length L
    credits L to each of its sites, and counts there once if it starts at the first site and once if it
    ends at the last.  -> (per site (sl, cens), the sum of L^2 over all runs)."""
    V = len(cols)
    res = [[0, 0] for _ in range(V)]
    sq = 0
    n = len(cols[0]) if V else 0
    for u in range(n):
        for v in range(u + 1, n):
            k = 0
            while k < V:
                if cols[k][u] != cols[k][v]:
                    k += 1
                    continue
                e = k
                while e + 1 < V and cols[e + 1][u] == cols[e + 1][v]:
                    e += 1
                L = e - k + 1
                sq += L * L
                for j in range(k, e + 1):
                    res[j][0] += L
                    res[j][1] += (k == 0) + (e == V - 1)
                k = e + 1
    return [tuple(r) for r in res], sq


def pooled_sites(ints, seg, pm, n, beg, end):
    """[(row, column)] of a chain: segregating rows of [beg, end) whose count m inside pm (n samples) has
    1 <= m <= n - 1."""
    rows = (beg + np.flatnonzero(seg[beg:end])).tolist()
    return [(r, ints[r] & pm) for r in rows if 1 <= bin(ints[r] & pm).count("1") <= n - 1]


def ref_xpnsl(types, flags, pop_masks, pop_n, wins, max_sites, chain=chain_sums):
    """n_var[nw, pairs] i32, row[nw, pairs, max_sites] i32, m and cens[nw, pairs, max_sites, 2] i32,
    sl[nw, pairs, max_sites, 2] i64.  A window with beg >= end, or outside the rows, is the empty window; a
    chain with more than max_sites pooled sites writes every slot as unused."""
    ints = row_ints(types)
    seg = (np.asarray(flags) & SEG) > 0
    L, nw, prs = len(seg), len(wins), pairs_of(len(pop_masks))
    n_var = np.zeros((nw, len(prs)), np.int32)
    row = np.full((nw, len(prs), max_sites), -1, np.int32)
    m = np.zeros((nw, len(prs), max_sites, 2), np.int32)
    sl = np.zeros((nw, len(prs), max_sites, 2), np.int64)
    cens = np.zeros((nw, len(prs), max_sites, 2), np.int32)
    for w, (beg, end) in enumerate(wins):
        if beg >= end or beg < 0 or end > L:
            continue
        for p, (i, j) in enumerate(prs):
            site = pooled_sites(ints, seg, pop_masks[i] | pop_masks[j], pop_n[i] + pop_n[j], beg, end)
            V = n_var[w, p] = len(site)
            if V == 0 or V > max_sites:
                continue
            row[w, p, :V] = [r for r, _ in site]
            for s, pm in enumerate((pop_masks[i], pop_masks[j])):
                res = chain([local_bits(x, pm) for _, x in site])
                m[w, p, :V, s] = [bin(x & pm).count("1") for _, x in site]
                sl[w, p, :V, s] = [r[0] for r in res]
                cens[w, p, :V, s] = [r[1] for r in res]
    return n_var, row, m, sl, cens


def value_text(n0, n1, sl0, sl1):
    """The printed value: the unstandardised XP-nSL, positive when side 0 carries the longer tracts."""
    c0, c1 = n0 * (n0 - 1) // 2, n1 * (n1 - 1) // 2
    if c0 == 0 or c1 == 0 or sl0 == 0 or sl1 == 0:
        return "NA"
    return "%.5f" % math.log((float(sl0) / float(c0)) / (float(sl1) / float(c1)))


def _agreeing(n, m):
    return m * (m - 1) // 2 + (n - m) * (n - m - 1) // 2


# ---- CPU tests ---------------------------------------------------------------------------
SIDES = [(1, 1), (1, 5), (2, 2), (2, 3), (3, 1), (4, 6), (6, 6), (8, 3), (5, 12), (12, 12)]


@pytest.mark.parametrize("n0,n1", SIDES, ids=[f"{a}x{b}" for a, b in SIDES])
def test_checker_agrees_with_the_run_decomposition(n0, n1):
    """Random and founder-structured pooled chains: the literal definition, its bit-parallel form and the
    run decomposition give the same numbers per side; a side's sums are its runs' squared lengths;
    A_s <= sl_s <= A_s V; cens at the first and last site is at least the agreeing pairs' count there."""
    rng = np.random.default_rng(4000 + 16 * n0 + n1)
    n = n0 + n1
    seen_mono, seen_long, seen_twice = 0, 0, 0
    for trial in range(300):
        V = int(rng.integers(0, 24))
        if trial % 2:
            cols = _founder_cols(rng, V, n, int(rng.integers(2, 5)), int(rng.integers(3, 12)))
        else:
            cols = [[int(x) for x in rng.integers(0, 2, n)] for _ in range(V)]
        cols = [c for c in cols if 0 < sum(c) < n]   # pooled sites only: a side may be monomorphic
        V = len(cols)
        for s, (lo, ns) in enumerate(((0, n0), (n0, n1))):
            side = [c[lo:lo + ns] for c in cols]
            a, b = chain_scalar(side), chain_sums(side)
            r, sq = chain_runs(side)
            assert a == b == r, (n0, n1, s, trial, cols)
            assert sum(x[0] for x in a) == sq
            for k, (sl, cens) in enumerate(a):
                ms = sum(side[k])
                A = _agreeing(ns, ms)
                assert A <= sl <= A * V and 0 <= cens <= 2 * A
                if k == 0 or k == V - 1:
                    assert cens >= A
                seen_mono += ms in (0, ns) and ns > 1
                seen_long += sl > 3 * A
                seen_twice += cens > A and 0 < k < V - 1
    if max(n0, n1) > 2:
        assert seen_mono > 10 and seen_long > 10 and seen_twice > 0


HAND_TYPES = np.array([0b00011, 0b11111, 0b01001, 0b01000, 0b10101, 0b11000, 0b00110, 0b11011], np.uint64)
HAND_FLAGS = np.array([COUNTED | SEG, COUNTED | SEG, COUNTED] + [COUNTED | SEG] * 5, np.uint8)
HAND_MASKS, HAND_N = [0b00111, 0b11000], [3, 2]
HAND_WINS = [(0, 8), (5, 8), (2, 2), (1, 3)]
HAND_WANT = {   # window -> [(row, m0, m1, sl0, sl1, cens0, cens1)] of the one pair
    0: [(0, 2, 0, 2, 1, 1, 1), (3, 0, 1, 6, 0, 1, 0), (4, 2, 1, 3, 0, 0, 0), (5, 0, 2, 6, 3, 0, 1), (6, 2, 0, 2, 3, 0, 1),
        (7, 2, 2, 1, 3, 1, 1)],
    1: [(5, 0, 2, 4, 3, 3, 2), (6, 2, 0, 2, 3, 1, 2), (7, 2, 2, 1, 3, 1, 2)],
    2: [], 3: [],
}


def _hand_made_expectations(n_var, row, m, sl, cens, max_sites):
    """Side 0 is samples 0..2 (C_0 = 3), side 1 samples 3 and 4 (C_1 = 1); a row is written s4 s3 s2 s1 s0.
    Row 1 (11111) is fixed in the pooled five samples, m = 5 > 4: not a pooled site.  Row 2 is not
    segregating.  Window [0, 8) has the pooled sites rows 0, 3, 4, 5, 6, 7 (V = 6, k = 0..5):
      row 0 = 00 011   side 1 monomorphic            row 3 = 01 000   side 0 monomorphic
      row 4 = 10 101   both vary                     row 5 = 11 000   both monomorphic, a fixed difference
      row 6 = 00 110   side 1 monomorphic            row 7 = 11 011   side 1 monomorphic
    Side 0's columns (s2 s1 s0) are 011, 000, 101, 000, 110, 011.  Per pair, A = agrees, D = not:
      (0,1)  A A D A D A   runs [0,1] of 2 (reaches the first site), [3] of 1, [5] of 1 (reaches the last)
      (0,2)  D A A A D D   run [1,3] of 3
      (1,2)  D A D A A D   runs [1] of 1, [3,4] of 2
    k = 0: (0,1) 2, first -> sl 2, cens 1.   k = 1: 2 + 3 + 1 = 6, (0,1) first -> cens 1.   k = 2: (0,2) 3.
    k = 3: 1 + 3 + 2 = 6.   k = 4: (1,2) 2.   k = 5: (0,1) 1, last -> cens 1.   The sums add to
    20 = 4 + 1 + 1 + 9 + 1 + 4, the runs' squares.
    Side 1's one pair (3,4) has the columns 00, 01, 10, 11, 00, 11: A D D A A A, runs [0] of 1 (first) and
    [3,5] of 3 (last): sl 1, 0, 0, 3, 3, 3 and cens 1, 0, 0, 1, 1, 1.  The value at k = 0 is
    log((2 / 3) / (1 / 1)); at k = 1 side 1's sum is 0 (two samples that differ): NA.

    Window [5, 8) is rows 5, 6, 7 (V = 3).  Side 0: 000, 110, 011: (0,1) A D A, (0,2) A D D, (1,2) A A D.
    k = 0: 1 + 1 + 2 = 4, all three reach the first site: cens 3.   k = 1: (1,2) 2, first: cens 1.
    k = 2: (0,1) 1, last: cens 1.   Side 1: 11, 00, 11: the pair agrees from edge to edge, so L = 3 at
    every site and it counts twice in cens everywhere.
    Window (2, 2) is empty; window [1, 3) holds rows 1 and 2 only: no pooled site."""
    for w, want in HAND_WANT.items():
        assert n_var[w, 0] == len(want)
        if len(want) > max_sites:
            want = []
        full = want + [(-1, 0, 0, 0, 0, 0, 0)] * (max_sites - len(want))
        got = [(int(row[w, 0, k]), *m[w, 0, k].tolist(), *sl[w, 0, k].tolist(), *cens[w, 0, k].tolist()) for k in range(max_sites)]
        assert got == full, (w, got, full)


def test_checker_on_a_hand_made_window():
    for max_sites in (0, 3, 5, 6, 9):   # 3 and 5: the whole-batch chain does not fit and writes nothing
        for chain in (chain_sums, chain_scalar):
            got = ref_xpnsl(HAND_TYPES, HAND_FLAGS, HAND_MASKS, HAND_N, HAND_WINS, max_sites, chain)
            _hand_made_expectations(*got, max_sites)
    assert value_text(3, 2, 2, 1) == "%.5f" % math.log(2.0 / 3.0) and value_text(3, 2, 6, 0) == "NA"
    assert value_text(3, 1, 6, 0) == "NA" == value_text(1, 3, 0, 6) and value_text(2, 2, 0, 1) == "NA"


def test_xpnsl_option_parses():
    base = ["-f", "ref.fa", "-w", "10"]
    for o_args, want in (([], 0), (["-o", "1"], 1), (["-o", "2"], 2), (["--hfs", "--nsl"], 0), (["-k", "3"], 0)):
        plain = opt.parse_args("haplo", base + o_args + ["in.bam", "chr1:1-500"])
        assert (plain.xpnsl, plain.output) == (0, want)
        for argv in (base + o_args + ["--xpnsl", "in.bam", "chr1:1-500"], ["--xpnsl"] + base + o_args + ["in.bam", "chr1:1-500"],
                     base + o_args + ["in.bam", "--xpnsl", "chr1:1-500"], base + o_args + ["in.bam", "chr1:1-500", "--xpnsl"]):
            o = opt.parse_args("haplo", argv)
            assert o.xpnsl == 1 and (o.hfs, o.nsl) == (plain.hfs, plain.nsl)
            o.xpnsl = 0
            assert o == plain   # every other field as without the token
    both = opt.parse_args("haplo", base + ["--hfs", "--nsl", "--xpnsl", "in.bam", "chr1"])
    assert (both.hfs, both.nsl, both.xpnsl) == (1, 1, 1)
    # only haplo has it
    for cmd in ("nucdiv", "sfs", "ld", "diverge", "snp", "tree"):
        assert opt.parse_args(cmd, base + ["--xpnsl", "in.bam", "chr1"]).xpnsl == 0
    with pytest.raises(opt.PopbamError, match="Not a valid output option"):
        opt.parse_args("haplo", base + ["-o", "3", "--xpnsl", "in.bam", "chr1"])


def test_native_xpnsl_errors_match_the_python_cli(capsys):
    """Error-text parity only: a bad haplo argv that also carries --xpnsl fails alike in both command lines.
    That the native binary knows the option is shown by test_xpnsl_command_line_on_a_golden_bam."""
    d = fixtures.load_case("g01_base")["dir"]
    ref, bam = os.path.join(d, "ref.fa"), os.path.join(d, "in.bam")
    for extra, msg in {"-o 3 --xpnsl": "Not a valid output option", "--xpnsl -o -1 --hfs --nsl": "Not a valid output option"}.items():
        argv = ["haplo", "-f", ref] + extra.split() + [bam, "chr1"]
        rc, out, err = _native(argv)
        prc = cli.main(argv)
        pe = capsys.readouterr()
        assert rc == prc == 1 and out == "" == pe.out, argv
        assert err == pe.err and msg in err, (argv, err, pe.err)


def test_xpnsl_is_exported():
    from popbam_amd import _lib, workload
    assert "pbg_window_xpnsl" in _lib.EXPORTS and hasattr(workload, "Xpnsl")
    # a bit of pbg_cmd.output, no new field: a program compiled against the header before it keeps running
    assert _lib.PBG_HAPLO_XPNSL == 8 and ("hfs", C.c_int32) == _lib.PbgCmd._fields_[-1]
    assert C.sizeof(_lib.PbgXpnslOpts) == 8 and [f for f, _ in _lib.PbgXpnslOut._fields_] == list(NAMES)


# ---- GPU tests ---------------------------------------------------------------------------
def _check_against_ref(ctx, rows, types, flags, masks, wins, what=""):
    pop_n = [bin(m).count("1") for m in masks]
    got, ms = _run_sized(ctx, rows, len(flags), wins)
    _assert_same(got, ref_xpnsl(types, flags, masks, pop_n, wins, ms), what)
    return got, ms


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_xpnsl_matches_the_checker_on_called_rows(gpu_lib, name):
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    wins = _windows(N_SITES, name not in WIDE)
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins, name)
    assert ms > 20 and sl.max() > 0 and n_var.shape[1] == len(pairs_of(len(masks)))
    assert not n_var[[3, 5]].any() and (row[[3, 5]] == -1).all() and not sl[[3, 5]].any() and not cens[[3, 5]].any()
    # both kinds of site are there: a side monomorphic at a pooled site, and both sides variable
    pop_n = [bin(x).count("1") for x in masks]
    p = 1 if name == "n14one" else 0   # a pair with two samples or more on each side
    i, j = pairs_of(len(masks))[p]
    V = n_var[0, p]
    m0, m1 = m[0, p, :V, 0], m[0, p, :V, 1]
    assert (((m0 == 0) | (m0 == pop_n[i])) & (m1 > 0) & (m1 < pop_n[j])).any()
    assert ((m0 > 0) & (m0 < pop_n[i]) & ((m1 == 0) | (m1 == pop_n[j]))).any()


@pytest.mark.gpu
def test_xpnsl_on_the_hand_made_window(gpu_lib):
    ctx, params, rows = _crafted(5, HAND_MASKS, HAND_TYPES, HAND_FLAGS)
    for max_sites in (0, 3, 5, 6, 9):
        _hand_made_expectations(*_run_xpnsl(ctx, rows, len(HAND_FLAGS), HAND_WINS, max_sites), max_sites)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n24p3", "n14one", "n126p3"])
def test_xpnsl_sites_are_those_of_nsl_on_the_merged_population(gpu_lib, name):
    """For each pair, n_var and row equal pbg_window_nsl's in a second context whose one population is
    pm_i | pm_j, and the two sides' counts add to that call's m."""
    from popbam_amd import _lib
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    wins = _windows(N_SITES, False)[:14]
    (n_var, row, m, sl, cens), ms = _run_sized(ctx, rows, N_SITES, wins)
    for p, (i, j) in enumerate(pairs_of(len(masks))):
        c2 = _lib.Context(_params(n, [masks[i] | masks[j]]), 0)
        assert c2.row_bytes == ctx.row_bytes
        g = _run_nsl(c2, rows, N_SITES, wins, ms)
        assert np.array_equal(g[0][:, 0], n_var[:, p]) and np.array_equal(g[1][:, 0], row[:, p]), (name, i, j)
        assert np.array_equal(g[2][:, 0], m[:, p].sum(axis=-1)), (name, i, j)
        c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n0,n1", [(20, 7), (6, 2), (70, 3)], ids=["20x7", "6x2", "70x3"])
def test_xpnsl_with_side_1_monomorphic_everywhere(gpu_lib, n0, n1):
    """Every sample of side 1 copies sample 0 of side 0, so side 1 is monomorphic at every row and the
    pooled sites are exactly side 0's variable sites.  Side 0's numbers (the pair loop) are then
    pbg_window_nsl's for population 0 with the classes added, and side 1's (the shortcut at every site)
    are C_1 V and 2 C_1."""
    L, n = 3000, n0 + n1
    rng = np.random.default_rng(50 + n)
    side0 = _founder_types(rng, L, n0, 5) if n0 > 64 else rng.integers(0, 1 << n0, L, dtype=np.uint64)
    ints = row_ints(side0)
    ints = [x | (((1 << n1) - 1) << n0 if x & 1 else 0) for x in ints]
    types = np.array([[x & ((1 << 64) - 1), x >> 64] for x in ints], np.uint64)
    types = types if n > 64 else types[:, 0].copy()
    flags = np.where(rng.random(L) < 0.5, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = _blocks([n0, n1])
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (0, 64), (100, 1100), (7, 9), (2000, 2999), (1500, 1500)]
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins, (n0, n1))
    g, gms = _run_sized(ctx, rows, L, wins, run=_run_nsl)
    assert gms == ms > 100 and np.array_equal(g[0][:, 0], n_var[:, 0]) and not g[0][:, 1].any()
    assert np.array_equal(g[1][:, 0], row[:, 0]) and np.array_equal(g[2][:, 0], m[:, 0, :, 0])
    assert np.array_equal(g[3][:, 0].sum(axis=-1), sl[:, 0, :, 0])
    assert np.array_equal(g[4][:, 0].sum(axis=-1), cens[:, 0, :, 0])
    c1 = n1 * (n1 - 1) // 2
    for w in range(len(wins)):
        V = n_var[w, 0]
        assert ((m[w, 0, :V, 1] == 0) | (m[w, 0, :V, 1] == n1)).all()
        assert (sl[w, 0, :V, 1] == c1 * V).all() and (cens[w, 0, :V, 1] == 2 * c1).all()
    ctx.close()


FOUNDER = [(12, 3, [6, 6]), (40, 4, [20, 20]), (96, 5, [48, 24, 24])]   # (samples, founders, population sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("n,founders,sizes", FOUNDER, ids=[f"n{a}" for a, _, _ in FOUNDER])
def test_xpnsl_on_founder_rows(gpu_lib, n, founders, sizes):
    """Long identical tracts; windows inside one stretch of 64 rows hold pairs that are identical across
    the whole window, counted twice in cens; windows that start and end inside a 16-byte word."""
    L = 2400
    rng = np.random.default_rng(200 + n)
    types = _founder_types(rng, L, n, founders)
    flags = np.where(rng.random(L) < 0.3, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = _blocks(sizes)
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (0, 64), (64, 128), (30, 100), (100, 612), (1001, 2103), (2391, L), (7, 8), (65, 127), (3, 1027)]
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins, n)
    assert n_var[0].min() > 100
    for w in (1, 2, 8):   # one stretch: some pair of each side agrees at every site of the window
        for p in range(n_var.shape[1]):
            V = n_var[w, p]
            assert V > 2 and (cens[w, p, :V] >= 2).all()
            assert (sl[w, p, V // 2] >= V).all()   # a tract that spans the window counts V at each of its sites
    ctx.close()


@pytest.mark.gpu
def test_xpnsl_sides_of_one_two_and_three(gpu_lib):
    """A side of one sample has no pair (C = 0, sl = 0, the value NA); two samples are one pair, whose sum
    is 0 where they differ (NA there) and positive where they agree."""
    L = 1500
    rng = np.random.default_rng(23)
    types = rng.integers(0, 1 << 12, L, dtype=np.uint64)
    flags = np.where(rng.random(L) < 0.5, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = [0b000000000001, 0b000000000110, 0b000000111000, 0b111111000000]   # 1, 2, 3 and 6 samples
    pop_n = [1, 2, 3, 6]
    ctx, params, rows = _crafted(12, masks, types, flags)
    wins = [(0, L), (10, 700), (701, 705)]
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins)
    prs = pairs_of(4)
    for p, (i, j) in enumerate(prs):
        V = n_var[0, p]
        assert V > 100
        if i == 0:   # side 0 is one sample
            assert not sl[:, p, :, 0].any() and not cens[:, p, :, 0].any()
            assert all(value_text(1, pop_n[j], *sl[0, p, k].tolist()) == "NA" for k in range(V))
    p12 = prs.index((1, 2))
    V = n_var[0, p12]
    differ = m[0, p12, :V, 0] == 1
    assert differ.any() and (~differ).any()
    assert not sl[0, p12, :V, 0][differ].any() and (sl[0, p12, :V, 0][~differ] > 0).all()
    texts = [value_text(2, 3, *sl[0, p12, k].tolist()) for k in range(V)]
    assert all(t == "NA" for t, d in zip(texts, differ) if d) and any(t != "NA" for t in texts)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_xpnsl_partial_last_word(gpu_lib, n, words):
    """Windows that end at n_rows = L, no multiple of the rows per 16-byte word; the rows sit in a larger
    buffer of 0xFF bytes.  Every row is segregating, so with 513 words the forward queue wraps and the
    backward trips of 64 sites start in the middle of the forward ones; samples copy founders over
    stretches of 200 rows, so tracts cross the trips in both directions."""
    L, more = partial_rows(n, words)
    rng = np.random.default_rng(n)
    sizes = [n // 3, n // 3, n - 2 * (n // 3)]
    masks = _blocks(sizes)
    full = (1 << n) - 1
    ints = []
    for r0 in range(0, L, 200):
        src = rng.integers(0, 4, n)
        for _ in range(min(200, L - r0)):
            fb = rng.integers(0, 2, 4)
            x = sum(int(fb[src[s]]) << s for s in range(n))
            ints.append(x if 0 < x < full else 0b0110)
    types = np.array([[x & ((1 << 64) - 1), x >> 64] for x in ints], np.uint64)
    types = types if n > 64 else types[:, 0].copy()
    flags = np.full(L, COUNTED | SEG, np.uint8)
    ctx, params, rows = _crafted(n, masks, types, flags)
    big = _padded(rows)
    assert words is None or L == words * (16 // ctx.row_bytes) + 3
    wins = [(3, L), (0, L), (L - 1, L), (L - 9, L), (1, 2), (L - 2, L)] + more
    if L > 3000:   # the checker's time: the long chains once, the rest short
        wins = [(3, L), (L - 1, L), (L - 9, L), (1, 2), (L - 2, L), (L - 1500, L)] + more
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, big, types, flags, masks, wins, (n, words))
    assert n_var[0].max() > (L - 3) // 2 and sl[0].max() > 64 * 3   # tracts longer than a backward trip
    V = n_var[0, 0]
    assert row[0, 0, V - 1] <= L - 1 and row[0, 0, 0] >= 3
    ctx.close()


@pytest.mark.gpu
def test_xpnsl_stride_edges(gpu_lib):
    """max_sites = the largest V; one less: that chain writes nothing and n_var stays; 1; NULL members."""
    from popbam_amd import workload
    ctx, params, rows, types, flags = _shape("n24p3")
    n, masks = SHAPES["n24p3"]
    pop_n = [8, 8, 8]
    wins = [(0, 4000), (100, 1100), (5, 5), (2000, 2300), (700, 703)]
    full, ms = _run_sized(ctx, rows, N_SITES, wins)
    n_var = full[0]
    assert ms == n_var.max() > 10
    _assert_same(full, ref_xpnsl(types, flags, masks, pop_n, wins, ms), "exact")
    less = _run_xpnsl(ctx, rows, N_SITES, wins, ms - 1)
    _assert_same(less, ref_xpnsl(types, flags, masks, pop_n, wins, ms - 1), "one less")
    big = np.argwhere(n_var == ms)
    assert len(big) >= 1
    for w, p in big.tolist():
        assert (less[1][w, p] == -1).all() and not less[2][w, p].any() and not less[3][w, p].any() and not less[4][w, p].any()
        assert less[0][w, p] == ms
    small = np.argwhere((n_var < ms) & (n_var > 0))[0]
    assert less[3][small[0], small[1]].any()
    one = _run_xpnsl(ctx, rows, N_SITES, wins, 1)   # only the chains of one site fit
    _assert_same(one, ref_xpnsl(types, flags, masks, pop_n, wins, 1), "one")
    assert (one[1][n_var != 1] == -1).all()
    more = _run_xpnsl(ctx, rows, N_SITES, wins, ms + 70)   # unused slots past one stride of lanes
    _assert_same(more, ref_xpnsl(types, flags, masks, pop_n, wins, ms + 70), "more")
    # row and m alone: no walk
    part = workload.Xpnsl(ctx, len(wins), ms)
    part.sl.fill_(9)
    part.cens.fill_(9)
    part.out.sl = part.out.cens = None
    part(rows, _wins_tensor(wins), N_SITES)
    ctx.sync_check()
    got = _arrays(part, NAMES)
    assert all(np.array_equal(got[k], full[k]) for k in (0, 1, 2)) and (got[3] == 9).all() and (got[4] == 9).all()


@pytest.mark.gpu
def test_xpnsl_argument_errors(gpu_lib):
    from popbam_amd import _lib, workload
    ctx, params, rows, types, flags = _shape("n12p2")
    wins = _wins_tensor([(0, 1000)])
    j = workload.Xpnsl(ctx, 1, 96)
    lib, s = ctx.lib, workload.stream_handle()
    r, w, o, out = rows.data_ptr(), wins.data_ptr(), C.byref(j.opts), C.byref(j.out)
    assert lib.pbg_window_xpnsl(None, r, N_SITES, w, 1, o, out, s) == _lib.PBG_E_ARG
    for args in ((None, N_SITES, w, 1, o, out), (r, N_SITES, None, 1, o, out), (r, N_SITES, w, 1, None, out),
                 (r, N_SITES, w, 1, o, None)):
        assert lib.pbg_window_xpnsl(ctx.h, *args, s) == _lib.PBG_E_ARG
        assert lib.pbg_last_error(ctx.h)
    bad = _lib.PbgXpnslOpts(-1, 0)
    assert lib.pbg_window_xpnsl(ctx.h, r, N_SITES, w, 1, C.byref(bad), out, s) == _lib.PBG_E_ARG
    assert b"max_sites" in lib.pbg_last_error(ctx.h)
    zero = _lib.PbgXpnslOpts(0, 0)
    for nm in NAMES[1:]:   # a per-site member with no room for a site
        one = _lib.PbgXpnslOut(j.n_var.data_ptr(), None, None, None, None)
        setattr(one, nm, getattr(j, nm).data_ptr())
        assert lib.pbg_window_xpnsl(ctx.h, r, N_SITES, w, 1, C.byref(zero), C.byref(one), s) == _lib.PBG_E_ARG
        assert b"max_sites" in lib.pbg_last_error(ctx.h)
    for nm in ("sl", "cens"):   # the backward walk reads the sites back through row
        one = _lib.PbgXpnslOut(j.n_var.data_ptr(), None, j.m.data_ptr(), None, None)
        setattr(one, nm, getattr(j, nm).data_ptr())
        assert lib.pbg_window_xpnsl(ctx.h, r, N_SITES, w, 1, o, C.byref(one), s) == _lib.PBG_E_ARG
        assert b"row" in lib.pbg_last_error(ctx.h)
    # the count-only call with NULL per-site members, and no output at all
    for members in ((j.n_var.data_ptr(), None, None, None, None), (None,) * 5):
        assert lib.pbg_window_xpnsl(ctx.h, r, N_SITES, w, 1, C.byref(zero), C.byref(_lib.PbgXpnslOut(*members)), s) == _lib.PBG_OK
    # no window: PBG_OK, nothing written
    assert workload.Xpnsl(ctx, 0, 8).run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    # one population has no pair: PBG_OK, nothing written
    c1 = _lib.Context(_params(12, [0b111111111111]), 0)
    j1 = workload.Xpnsl(c1, 1, 8)
    assert j1.n_pairs == 0 and j1.n_var.shape == (1, 0) and j1.run(rows, wins, N_SITES) == _lib.PBG_OK
    c1.sync_check()
    c1.close()
    # pop_n that is not the masks' popcount
    p2 = _params(12, _blocks([6, 6]))
    p2.pop_n[1] = 5
    c2 = _lib.Context(p2, 0)
    j2 = workload.Xpnsl(c2, 1, 96)
    assert j2.run(rows, wins, N_SITES) == _lib.PBG_E_ARG and b"pop_n" in lib.pbg_last_error(c2.h)
    c2.close()
    # a window past the rows is never read: an empty window's outputs, reported by pbg_check
    over = workload.Xpnsl(ctx, 3, 96)
    for nm in NAMES:
        getattr(over, nm).fill_(7)
    assert over.run(rows, _wins_tensor([(0, N_SITES + 1), (0, 1000), (-1, 10)]), N_SITES) == _lib.PBG_OK
    assert lib.pbg_check(ctx.h, None) == _lib.PBG_E_RANGE
    assert j.run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    for w_ in (0, 2):
        assert not over.n_var[w_].any() and (over.row[w_] == -1).all()
        assert not over.m[w_].any() and not over.sl[w_].any() and not over.cens[w_].any()
    for nm in NAMES:
        assert getattr(over, nm)[1].cpu().numpy().tobytes() == getattr(j, nm)[0].cpu().numpy().tobytes(), nm
    assert 0 < j.n_var[0].min() and j.n_var[0].max() <= 96 and j.sl[0].max() > 0


@pytest.mark.gpu
def test_xpnsl_is_deterministic_and_interleaves_with_the_other_calls(gpu_lib):
    """Statistics, XP-nSL, nSL, XP-nSL, Rmin, XP-nSL, statistics, with the same pointers on one context and
    stream: each equals its own stand-alone run on a fresh context byte for byte, and two XP-nSL runs give
    equal bytes."""
    from popbam_amd import workload
    others = lambda wins: {"rmin": (lambda ctx: workload.Rmin(ctx, len(wins), 1, 16), workload.Rmin.NAMES)}   # noqa: E731
    _interleaving("xpnsl", ("Xpnsl", "Nsl"), others, ("xpnsl", "nsl", "xpnsl", "rmin", "xpnsl"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12p2", "n40p2i", "n126p3"])
def test_xpnsl_under_the_bounds_build(gpu_lib, tmp_path, name):
    """Called rows through the PBG_BOUNDS build (a fresh process): the same rows and the checker's numbers,
    and the error word stays 0."""
    assert os.path.exists(BOUNDS_LIB), "the bounds build is not there: the Makefile's `bounds` target builds it"
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    wins = _windows(N_SITES, False)
    pop_n = [bin(m).count("1") for m in masks]
    ints, seg = row_ints(types), (np.asarray(flags) & SEG) > 0
    ms = max(len(pooled_sites(ints, seg, masks[i] | masks[j], pop_n[i] + pop_n[j], a, b)) for a, b in wins if a < b
             for i, j in pairs_of(len(masks)))
    (brows, got), = _bounds_child(tmp_path, [dict(call="Xpnsl", n=n, masks=masks, wins=wins, n_rows=N_SITES, max_sites=ms,
                                                  synth=(N_SITES, 10, SEED + n))])
    assert np.array_equal(brows, rows.cpu().numpy())
    _assert_same(got, ref_xpnsl(types, flags, masks, pop_n, wins, ms), "bounds")


# ---- command lines -----------------------------------------------------------------------
def _split_xpnsl(line, pops):
    """(the part before the xpnsl columns, {(popI, popJ): [(pos, mI, mJ, value text, c)]})."""
    at = line.index("\txpnsl[")
    f = line[at + 1:].split("\t")
    prs = pairs_of(len(pops))
    assert len(f) == 2 * len(prs), f
    ext = {}
    for p, (i, j) in enumerate(prs):
        assert f[2 * p] == f"xpnsl[{pops[i]},{pops[j]}]:", f
        toks = [] if f[2 * p + 1] == "NA" else [t.split(":") for t in f[2 * p + 1].split(",")]
        assert all(len(t) == 5 for t in toks), f
        ext[(i, j)] = [(int(a), int(b), int(c), v, int(d)) for a, b, c, v, d in toks]
    return line[:at], ext


def _check_text(ours, plain, pops, pop_n, res, pos0, what):
    """Every line: the plain line, then per pair the checker's tokens."""
    n_var, row, m, sl, cens = res
    lines, plain_lines = ours.splitlines(), plain.splitlines()
    assert len(lines) == len(plain_lines) == len(n_var) > 0
    values = 0
    for w, (line, pl) in enumerate(zip(lines, plain_lines)):
        head, ext = _split_xpnsl(line, pops)
        assert head == pl, (what, w)
        for p, (i, j) in enumerate(pairs_of(len(pops))):
            V = n_var[w, p]
            want = [(int(row[w, p, k]) + pos0 + 1, int(m[w, p, k, 0]), int(m[w, p, k, 1]),
                     value_text(pop_n[i], pop_n[j], *sl[w, p, k].tolist()), int(cens[w, p, k].sum())) for k in range(V)]
            assert ext[(i, j)] == want, (what, w, i, j)
            values += sum(t[3] != "NA" for t in want)
    return values


CMD_CASES = [(nm, extra) for nm in ("g01_base", "g03_threepops")
             for extra in ((), ("-o", "1"), ("-o", "2"), ("--hfs",), ("--nsl",), ("--hfs", "--nsl"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", CMD_CASES, ids=[nm + "".join(e).replace("-", "") for nm, e in CMD_CASES])
def test_xpnsl_command_line_on_a_golden_bam(gpu_lib, name, extra):
    """`popbam haplo -w 1 [-o N] [--hfs] [--nsl] --xpnsl` through cli.run and the native binary: the same
    text from both; the part before the xpnsl columns is the run without --xpnsl (the golden text where
    there is one); the tokens are the checker's and the library call's on the stream's rows."""
    import torch
    from popbam_amd import _lib, engine, workload
    case = fixtures.load_case(name)
    d = case["dir"]
    args = ["haplo", "-w", "1"] + list(extra)
    base = ["haplo", "-f", os.path.join(d, "ref.fa"), "-w", "1"] + list(extra)
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run(base[0], base[1:] + tail)
    ours = cli.run(base[0], base[1:] + ["--xpnsl"] + tail)
    rc, nat, err = _native(base[:1] + ["--xpnsl"] + base[1:] + tail)   # the token in front here, at the end there
    assert rc == 0, err
    assert nat == ours
    gold = [c for c in case["meta"]["cases"] if c["args"] == args]
    assert bool(gold) == ("--hfs" not in extra and "--nsl" not in extra)
    if gold:
        assert plain == fixtures.golden_text(name, gold[0]["stdout"])
    st = harness.Setup(name, args + ["--xpnsl"], "chr1")
    assert st.opts.xpnsl == 1 and st.opts.output == (int(extra[1]) if "-o" in extra else 0)
    ctx = _lib.Context(engine.make_params(st.opts, st.sm), 0)
    kb = st.kbatch
    ref = np.ascontiguousarray(kb["ref"], dtype=np.uint8)
    k = np.ascontiguousarray(kb["k"], dtype=np.uint8 if ctx.k_bytes == 1 else np.uint16)
    rq = np.ascontiguousarray(kb["rmsq"], dtype=np.uint32)
    keys = np.ascontiguousarray(kb["keys"], dtype=np.uint16)
    L = len(ref)
    cmd = engine._Cmd(st.opts, st.sm, st.chr, st.beg, st.end)
    assert cmd.c.output == st.opts.output | _lib.PBG_HAPLO_XPNSL | (_lib.PBG_HAPLO_NSL if "--nsl" in extra else 0)
    rows = torch.zeros(L * ctx.row_bytes, dtype=torch.uint8, device="cuda")
    with _lib.Stream(ctx, [cmd.c], 0, L) as s:
        s.push(_lib.PbgPileup(L, 0, ref.ctypes.data, k.ctypes.data, rq.ctypes.data, None, keys.ctypes.data))
        s.finish()
        text = s.text(0)
        s.rows_into(rows.data_ptr(), rows.numel())
    assert text == ours
    wins = workload.reference_windows(st.beg, st.end, st.opts.win_size)
    types, flags = harness.rows_to_sites(rows.cpu().numpy(), ctx.row_bytes, L, st.sm.n)
    got, ms = _run_sized(ctx, rows, L, wins)
    res = ref_xpnsl(types, flags, st.masks, st.pop_n, wins, ms)
    _assert_same(got, res, name)
    assert res[0].max() > 1
    assert _check_text(ours, plain, st.sm.pops, st.pop_n, got, 0, name) > 0   # rows are contig positions here
    ctx.close()


@pytest.mark.gpu
def test_xpnsl_appends_nothing_for_one_population(gpu_lib):
    d = fixtures.load_case("g14_onepop")["dir"]
    base = ["-f", os.path.join(d, "ref.fa"), "-w", "1"]
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run("haplo", base + tail)
    assert plain and cli.run("haplo", base + ["--xpnsl"] + tail) == plain
    rc, nat, err = _native(["haplo"] + base + ["--xpnsl"] + tail)
    assert rc == 0 and nat == plain, err
    with_nsl = cli.run("haplo", base + ["--nsl"] + tail)
    assert with_nsl != plain and cli.run("haplo", base + ["--nsl", "--xpnsl"] + tail) == with_nsl


def _stream_case(n, masks, L, W, output, hfs, seed):
    """Streams `haplo -w W` with the given output bits and hfs over a synthetic batch of n samples in the
    populations `masks`, pushed in several pieces, once without and once with PBG_HAPLO_XPNSL.  Checks the
    rows, the library call and every token against the checker; -> (text with the bit, population names,
    the checker's arrays, the number of tokens whose value is a number)."""
    import torch
    from popbam_amd import _lib, workload
    npops = len(masks)
    ctx = _lib.Context(_params(n, masks), 0)
    syn = workload.SynthPileup(ctx, L, 10, seed)
    hp = workload.HotPath(ctx, syn, [(0, L)], 0)
    hp.call()
    ctx.sync_check()
    host = hp.to_host()
    names = [f"p{i}" for i in range(npops)]
    keep = [b"chr1", (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)]), (C.c_char_p * npops)(*[x.encode() for x in names])]

    def run(out_bits):
        c = _lib.PbgCmd()
        c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq, c.hfs = 1, out_bits, 10, 10, 1, hfs   # PBG_CMD_HAPLO
        c.windowed, c.win_size, c.beg, c.end = 1, W, 0, L
        c.chr_name = keep[0]
        c.sample_names = C.cast(keep[1], C.POINTER(C.c_char_p))
        c.pop_names = C.cast(keep[2], C.POINTER(C.c_char_p))
        c.refid = b"ref"
        rows = torch.zeros_like(hp.rows)
        with _lib.Stream(ctx, [c], 0, L, 64 * 100) as st:
            st.push(_lib.PbgPileup(L, 0, host["ref"].data_ptr(), host["k"].data_ptr(), host["rmsq"].data_ptr(),
                                   host["block_off"].data_ptr(), host["keys"].data_ptr()))
            st.finish()
            text = st.text(0)
            st.rows_into(rows.data_ptr(), rows.numel())
        return text, rows

    plain, rows0 = run(output)
    ours, rows = run(output | _lib.PBG_HAPLO_XPNSL)
    assert torch.equal(rows, rows0) and torch.equal(rows, hp.rows)
    pop_n = [bin(m).count("1") for m in masks]
    wins = workload.reference_windows(0, L, W)
    types, flags = harness.rows_to_sites(rows.cpu().numpy(), ctx.row_bytes, L, n)
    got, ms = _run_sized(ctx, rows, L, wins)
    res = ref_xpnsl(types, flags, masks, pop_n, wins, ms)
    _assert_same(got, res, "stream")
    values = _check_text(ours, plain, names, pop_n, res, 0, "stream")
    ctx.close()
    return ours, names, res, values


@pytest.mark.gpu
@pytest.mark.parametrize("output,hfs,W", [(0, 0, 1000), (1, 1, 1000), (2 | 4, 0, 1000), (0, 0, 5)], ids=["o0", "o1hfs", "o2nsl", "w5"])
def test_xpnsl_on_a_synthetic_stream(gpu_lib, output, hfs, W):
    """A streamed run of `haplo -w W [-o N] [--hfs] [--nsl] --xpnsl` over a synthetic batch of 24 samples
    in three populations, pushed in several pieces: the line without its xpnsl columns is the stream's line
    without the bit, and the tokens are the checker's on the stream's rows.  With W = 5 the 3,200 windows
    are staged in two blocks (a block is 64 MiB of 256-site strides: 2,426 windows of three pairs)."""
    ours, names, res, values = _stream_case(24, _blocks([8, 8, 8]), 64 * 250, W, output, hfs, SEED + 5)
    assert values > 10


@pytest.mark.gpu
def test_xpnsl_stream_prints_na_for_small_sides(gpu_lib):
    """The product's text (format.cpp) for sides of 1, 2, 3 and 6 samples: every value of a pair with a
    one-sample side is NA (C = 0); in the pair of the two- and the three-sample side the value is NA
    exactly where the two samples differ (sl = 0) and a number elsewhere; the text holds no inf or nan."""
    masks = [0b000000000001, 0b000000000110, 0b000000111000, 0b111111000000]
    ours, names, res, values = _stream_case(12, masks, 64 * 250, 2000, 0, 0, SEED + 12)
    low = ours.lower()
    assert "inf" not in low and "nan" not in low and values > 10
    c0_na = sl0_na = numbers = 0
    for line in ours.splitlines():
        _, ext = _split_xpnsl(line, names)
        for j in (1, 2, 3):   # side 0 is one sample
            assert all(v == "NA" for _, _, _, v, _ in ext[(0, j)])
            c0_na += len(ext[(0, j)])
        for _, m_two, _, v, _ in ext[(1, 2)]:   # side 0 is two samples, side 1 three (always an agreeing pair)
            assert (v == "NA") == (m_two == 1), (m_two, v)
            sl0_na += v == "NA"
            numbers += v != "NA"
    assert c0_na > 100 and sl0_na > 10 and numbers > 10
