"""`haplo --nsl`: the per-site nSL tract sums (Ferrer-Admetlla et al. 2014) per window and population
(pbg_window_nsl, include/popbam_gpu.h; DESIGN.md "nSL").  The reference has no such output, so the
checker lives here.  `chain_scalar` restates the header's definition literally: per variable site and
sample pair, expand left and right while the pair agrees.  `chain_sums` is the same expansion with
the pairs of a site held as the bits of one Python integer, so that a window of thousands of sites
stays within seconds; `ref_nsl` lays its numbers out as the call does.  An independent form
(`chain_runs`: every pair's agreement sequence cut into maximal runs, each run's length credited to
its sites) checks both.  Every comparison is exact; the printed value is compared as the %.5f of
Python's math.log of the same two divisions."""
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
from tract_helpers import local_bits, row_ints, _assert_same, _founder_cols, _params, _shape, _windows, _run_nsl
from tract_helpers import _founder_types, _crafted, _padded, _interleaving, _bounds_child
from window_helpers import _arrays, _blocks, _native, _wins_tensor
from window_helpers import PARTIAL_WORD_CASES, partial_rows
from popbam_amd import cli
from popbam_amd import options as opt

_run_sized = partial(tract_helpers._run_sized, run=_run_nsl)


# ---- the checker -----------------------------------------------------------------------
def chain_scalar(cols):
    """The definition.  cols[k]: the population's bits at variable site k.  -> per site (sl0, sl1, cens0,
    cens1)."""
    V = len(cols)
    out = []
    for k in range(V):
        n = len(cols[k])
        sl, cens = [0, 0], [0, 0]
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
                sl[cols[k][u]] += l + r - 1
                cens[0] += l == k + 1
                cens[1] += r == V - k
        out.append((sl[0], sl[1], cens[0], cens[1]))
    return out


def _class_sets(cols):
    """Per site the pairs that agree with class 0 and with class 1, each as the bits of one integer
    (pair (u, v), u < v, in row-major order)."""
    if not cols:
        return []
    b = np.array(cols, dtype=bool)
    iu, iv = np.triu_indices(b.shape[1], 1)
    sets = []
    for c in (False, True):
        both = (b[:, iu] == c) & (b[:, iv] == c)
        packed = np.packbits(both, axis=1)
        sets.append([int.from_bytes(r.tobytes(), "big") for r in packed])
    return list(zip(*sets))


def chain_sums(cols):
    """chain_scalar with a site's pairs as one integer: the pairs of class c at k are expanded to the
    left and to the right while any of them still agrees; each step adds the survivors' count."""
    cls = _class_sets(cols)
    V = len(cls)
    agree = [a | b for a, b in cls]
    out = []
    for k in range(V):
        sl, cens = [0, 0], [0, 0]
        for c in (0, 1):
            for side, step in ((0, -1), (1, 1)):
                alive, j, tot = cls[k][c], k, 0
                while alive:
                    tot += alive.bit_count()
                    j += step
                    if j < 0 or j >= V:
                        cens[side] += alive.bit_count()   # the run reaches the window's first / last site
                        break
                    alive &= agree[j]
                sl[c] += tot   # the sum of l, then of r
            sl[c] -= cls[k][c].bit_count()   # L = l + r - 1
        out.append((sl[0], sl[1], cens[0], cens[1]))
    return out


def chain_runs(cols):
    """The independent form: every pair's agreement sequence cut into maximal runs; a run of length L
    credits L to each of its sites, in the class the pair has there.  -> (per site as chain_scalar, the
    sum of L^2 over all runs)."""
    V = len(cols)
    res = [[0, 0, 0, 0] for _ in range(V)]
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
                    res[j][cols[j][u]] += L
                    res[j][2] += k == 0
                    res[j][3] += e == V - 1
                k = e + 1
    return [tuple(r) for r in res], sq


def variable_sites(ints, seg, pm, n_i, beg, end):
    """[(row, column)] of a chain: segregating rows of [beg, end) with 1 <= m <= n_i - 1."""
    rows = (beg + np.flatnonzero(seg[beg:end])).tolist()
    return [(r, ints[r] & pm) for r in rows if 1 <= bin(ints[r] & pm).count("1") <= n_i - 1]


def ref_nsl(types, flags, pop_masks, pop_n, wins, max_sites, chain=chain_sums):
    """n_var[nw, np] i32, row and m[nw, np, max_sites] i32, sl[nw, np, max_sites, 2] i64,
    cens[nw, np, max_sites, 2] i32.  A window with beg >= end, or outside the rows, is the empty window; a
    chain with more than max_sites variable sites writes every slot as unused."""
    ints = row_ints(types)
    seg = (np.asarray(flags) & SEG) > 0
    L, nw, npop = len(seg), len(wins), len(pop_masks)
    n_var = np.zeros((nw, npop), np.int32)
    row = np.full((nw, npop, max_sites), -1, np.int32)
    m = np.zeros((nw, npop, max_sites), np.int32)
    sl = np.zeros((nw, npop, max_sites, 2), np.int64)
    cens = np.zeros((nw, npop, max_sites, 2), np.int32)
    for w, (beg, end) in enumerate(wins):
        if beg >= end or beg < 0 or end > L:
            continue
        for i, (pm, n_i) in enumerate(zip(pop_masks, pop_n)):
            site = variable_sites(ints, seg, pm, n_i, beg, end)
            V = n_var[w, i] = len(site)
            if V == 0 or V > max_sites:
                continue
            res = chain([local_bits(x, pm) for _, x in site])
            row[w, i, :V] = [r for r, _ in site]
            m[w, i, :V] = [bin(x).count("1") for _, x in site]
            sl[w, i, :V] = [r[:2] for r in res]
            cens[w, i, :V] = [r[2:] for r in res]
    return n_var, row, m, sl, cens


def value_text(n_i, m, sl0, sl1):
    """The printed value: the unstandardised nSL relative to the reference allele."""
    p0, p1 = (n_i - m) * (n_i - m - 1) // 2, m * (m - 1) // 2
    if p0 == 0 or p1 == 0:
        return "NA"
    return "%.5f" % math.log((float(sl0) / float(p0)) / (float(sl1) / float(p1)))


# ---- CPU tests ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 8, 12])
def test_checker_agrees_with_the_run_decomposition(n):
    """Random and founder-structured chains: the literal definition, its bit-parallel form and the run
    decomposition give the same numbers; the sums are the runs' squared lengths; P_c <= sl_c <= P_c V;
    cens at the first and last site is the agreeing pairs' count there."""
    rng = np.random.default_rng(3000 + n)
    seen_cens, seen_long = 0, 0
    for trial in range(400):
        V = int(rng.integers(0, 30))
        if trial % 2:
            cols = _founder_cols(rng, V, n, int(rng.integers(2, 5)), int(rng.integers(3, 12)))
        else:
            cols = [[int(x) for x in rng.integers(0, 2, n)] for _ in range(V)]
        cols = [c for c in cols if 0 < sum(c) < n]   # variable sites only
        V = len(cols)
        a, b = chain_scalar(cols), chain_sums(cols)
        r, sq = chain_runs(cols)
        assert a == b == r, (n, trial, cols)
        assert sum(x[0] + x[1] for x in a) == sq
        for k, (s0, s1, c0, c1) in enumerate(a):
            m = sum(cols[k])
            p0, p1 = (n - m) * (n - m - 1) // 2, m * (m - 1) // 2
            assert p0 <= s0 <= p0 * V and p1 <= s1 <= p1 * V
            assert 0 <= c0 <= p0 + p1 and 0 <= c1 <= p0 + p1
            if k == 0:
                assert c0 == p0 + p1
            if k == V - 1:
                assert c1 == p0 + p1
            seen_cens += (c0 > 0 and c1 > 0 and 0 < k < V - 1)
            seen_long += s0 + s1 > 3 * (p0 + p1)
    if n == 2:   # one pair, and every variable site splits it
        assert seen_long == 0
    else:
        assert seen_cens > 10 and seen_long > 10   # tracts censored on both sides, and long ones


HAND_TYPES = np.array([0b0010011, 0b0110001, 0b1111111, 0b0000011, 0b1000111, 0b1101111, 0b0010101], np.uint64)
HAND_FLAGS = np.array([COUNTED | SEG, COUNTED | SEG, COUNTED, COUNTED | SEG, COUNTED | SEG, COUNTED | SEG, COUNTED | SEG], np.uint8)
HAND_MASKS, HAND_N = [0b0001111, 0b1110000], [4, 3]
HAND_WINS = [(0, 7), (1, 6), (3, 3)]
HAND_WANT = {   # (window, population) -> [(row, m, sl0, sl1, cens0, cens1)]
    (0, 0): [(0, 2, 3, 1, 2, 0), (1, 1, 5, 0, 1, 0), (3, 2, 3, 2, 1, 0), (4, 3, 0, 5, 0, 1), (6, 2, 1, 2, 0, 2)],
    (0, 1): [(0, 1, 1, 0, 1, 0), (1, 2, 0, 2, 0, 0), (4, 1, 2, 0, 0, 0), (5, 2, 0, 2, 0, 1), (6, 1, 2, 0, 0, 1)],
    (1, 0): [(1, 1, 4, 0, 3, 0), (3, 2, 2, 2, 1, 1), (4, 3, 0, 4, 0, 3)],
    (1, 1): [(1, 2, 0, 2, 1, 0), (4, 1, 2, 0, 1, 0), (5, 2, 0, 1, 0, 1)],
    (2, 0): [], (2, 1): [],
}


def _hand_made_expectations(n_var, row, m, sl, cens, max_sites):
    """Population 0 is samples 0..3, population 1 samples 4..6.  Row 2 is not segregating.

    Population 0, window [0, 7): row 5 is 1111, not variable; the sites are rows 0, 1, 3, 4, 6 with
    columns (samples 3210) 0011, 0001, 0011, 0111, 0101.  Per pair, A = agrees (with its class), D = not:
      (0,1)  A1 D  A1 A1 D    runs [0] of 1, [2,3] of 2
      (0,2)  D  D  D  A1 A1   run [3,4] of 2, reaches the last site
      (0,3)  D  D  D  D  D
      (1,2)  D  A0 D  A1 D    runs [1] of 1, [3] of 1
      (1,3)  D  A0 D  D  A0   runs [1] of 1, [4] of 1 (reaches the last site)
      (2,3)  A0 A0 A0 D  D    run [0,2] of 3, reaches the first site
    site 0: class 0 (2,3): 3; class 1 (0,1): 1; both reach the first site.   site 1: class 0: 1 + 1 + 3.
    site 2: class 0: 3 (first); class 1 (0,1): 2.   site 3: class 1: 2 + 2 + 1, (0,2) reaches the last.
    site 4: class 0 (1,3): 1; class 1 (0,2): 2; both reach the last site.  The sums add to 22 = 1 + 4 + 4
    + 1 + 1 + 1 + 1 + 9, the runs' squares.

    Population 1, window [0, 7): row 3 is 000; the sites are rows 0, 1, 4, 5, 6 with columns (samples
    654) 001, 011, 100, 110, 001:
      (4,5)  D  A1 A0 D  D    one run [1,2] of 2 whose class changes inside it
      (4,6)  D  D  D  D  D
      (5,6)  A0 D  D  A1 A0   runs [0] of 1 (first), [3,4] of 2 (last)

    Window [1, 6) drops rows 0 and 6.  Population 0: columns 0001, 0011, 0111; (0,1) D A1 A1, (0,2) D D A1,
    (1,2) A0 D A1, (1,3) A0 D D, (2,3) A0 A0 D.  Population 1: columns 011, 100, 110; (4,5) A1 A0 D,
    (5,6) D D A1.  Window (3, 3) is empty."""
    for (w, i), want in HAND_WANT.items():
        assert n_var[w, i] == len(want)
        if len(want) > max_sites:
            want = []
        full = want + [(-1, 0, 0, 0, 0, 0)] * (max_sites - len(want))
        got = [(int(row[w, i, k]), int(m[w, i, k]), *sl[w, i, k].tolist(), *cens[w, i, k].tolist()) for k in range(max_sites)]
        assert got == full, (w, i, got, full)


def test_checker_on_a_hand_made_window():
    for max_sites in (0, 4, 5, 7):   # 4: the whole-batch chains do not fit and write nothing
        for chain in (chain_sums, chain_scalar):
            got = ref_nsl(HAND_TYPES, HAND_FLAGS, HAND_MASKS, HAND_N, HAND_WINS, max_sites, chain)
            _hand_made_expectations(*got, max_sites)
    assert value_text(4, 2, 3, 1) == "%.5f" % math.log(3.0) and value_text(4, 1, 5, 0) == "NA" == value_text(4, 3, 0, 5)


def test_nsl_option_parses():
    base = ["-f", "ref.fa", "-w", "10"]
    for o_args, want in (([], 0), (["-o", "1"], 1), (["-o", "2"], 2), (["--hfs"], 0), (["-k", "3"], 0)):
        plain = opt.parse_args("haplo", base + o_args + ["in.bam", "chr1:1-500"])
        assert (plain.nsl, plain.output) == (0, want)
        for argv in (base + o_args + ["--nsl", "in.bam", "chr1:1-500"], ["--nsl"] + base + o_args + ["in.bam", "chr1:1-500"],
                     base + o_args + ["in.bam", "--nsl", "chr1:1-500"], base + o_args + ["in.bam", "chr1:1-500", "--nsl"]):
            o = opt.parse_args("haplo", argv)
            assert o.nsl == 1
            o.nsl = 0
            assert o == plain   # every other field as without the token
    # only haplo has it
    for cmd in ("nucdiv", "sfs", "ld", "diverge", "snp", "tree"):
        assert opt.parse_args(cmd, base + ["--nsl", "in.bam", "chr1"]).nsl == 0
    with pytest.raises(opt.PopbamError, match="Not a valid output option"):
        opt.parse_args("haplo", base + ["-o", "3", "--nsl", "in.bam", "chr1"])


def test_native_nsl_errors_match_the_python_cli(capsys):
    d = fixtures.load_case("g01_base")["dir"]
    ref, bam = os.path.join(d, "ref.fa"), os.path.join(d, "in.bam")
    for extra, msg in {"-o 3 --nsl": "Not a valid output option", "--nsl -o -1 --hfs": "Not a valid output option"}.items():
        argv = ["haplo", "-f", ref] + extra.split() + [bam, "chr1"]
        rc, out, err = _native(argv)
        prc = cli.main(argv)
        pe = capsys.readouterr()
        assert rc == prc == 1 and out == "" == pe.out, argv
        assert err == pe.err and msg in err, (argv, err, pe.err)


def test_nsl_is_exported():
    from popbam_amd import _lib, workload
    assert "pbg_window_nsl" in _lib.EXPORTS and hasattr(workload, "Nsl")
    # a bit of pbg_cmd.output, no new field: a program compiled against the header before it keeps running
    assert _lib.PBG_HAPLO_NSL == 4 and ("hfs", C.c_int32) == _lib.PbgCmd._fields_[-1]
    assert C.sizeof(_lib.PbgNslOpts) == 8 and [f for f, _ in _lib.PbgNslOut._fields_] == list(NAMES)


# ---- GPU tests ---------------------------------------------------------------------------
def _check_against_ref(ctx, rows, types, flags, masks, wins, what=""):
    pop_n = [bin(m).count("1") for m in masks]
    got, ms = _run_sized(ctx, rows, len(flags), wins)
    _assert_same(got, ref_nsl(types, flags, masks, pop_n, wins, ms), what)
    return got, ms


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_nsl_matches_the_checker_on_called_rows(gpu_lib, name):
    from popbam_amd import workload
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    wins = _windows(N_SITES, name not in WIDE)
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins, name)
    assert ms > 20 and sl.max() > 0
    assert not n_var[[3, 5]].any() and (row[[3, 5]] == -1).all() and not sl[[3, 5]].any() and not cens[[3, 5]].any()
    # the variable sites are pbg_window_rmin's at min_freq = 1
    rm = workload.Rmin(ctx, len(wins), 1, 0)
    rm(rows, _wins_tensor(wins), N_SITES)
    ctx.sync_check()
    assert np.array_equal(rm.n_var.cpu().numpy(), n_var)
    # m is the popcount of the row inside the population
    ints = row_ints(types)
    for w, i in ((0, 0), (1, len(masks) - 1)):
        V = n_var[w, i]
        assert m[w, i, :V].tolist() == [bin(ints[r] & masks[i]).count("1") for r in row[w, i, :V].tolist()]
    if name == "n14one":
        assert n_var[:, 1].max() == 0   # one sample: no variable site at all


FOUNDER = [(12, 3, [6, 6]), (40, 4, [20, 20]), (96, 5, [48, 24, 24])]   # (samples, founders, population sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("n,founders,sizes", FOUNDER, ids=[f"n{a}" for a, _, _ in FOUNDER])
def test_nsl_on_founder_rows(gpu_lib, n, founders, sizes):
    """Long identical tracts; windows inside one stretch of 64 rows hold pairs that are identical across
    the whole window, censored on both sides; windows that start and end inside a 16-byte word."""
    L = 2400
    rng = np.random.default_rng(200 + n)
    types = _founder_types(rng, L, n, founders)
    flags = np.where(rng.random(L) < 0.3, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = _blocks(sizes)
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (0, 64), (64, 128), (30, 100), (100, 612), (1001, 2103), (2391, L), (7, 8), (65, 127), (3, 1027)]
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins, n)
    assert n_var[0].min() > 100
    for w in (1, 2, 8):   # one stretch: some pair agrees at every site of the window
        for i in range(len(masks)):
            V = n_var[w, i]
            assert V > 2 and (cens[w, i, :V] > 0).all()
            k = V // 2
            assert sl[w, i, k].sum() >= V   # a tract that spans the window counts V at each of its sites
    ctx.close()


@pytest.mark.gpu
def test_nsl_populations_of_two_and_three(gpu_lib):
    """Two samples are one pair, which every variable site splits: both sums are 0 and the value is NA."""
    L = 1500
    rng = np.random.default_rng(23)
    types = rng.integers(0, 1 << 12, L, dtype=np.uint64)
    flags = np.where(rng.random(L) < 0.5, COUNTED | SEG, COUNTED).astype(np.uint8)
    masks = [0b000000000011, 0b000000011100, 0b111111100000]   # 2, 3 and 7 samples
    ctx, params, rows = _crafted(12, masks, types, flags)
    wins = [(0, L), (10, 700), (701, 705)]
    (n_var, row, m, sl, cens), ms = _check_against_ref(ctx, rows, types, flags, masks, wins)
    assert n_var[0, 0] > 100 and not sl[:, 0].any() and not cens[:, 0].any() and (m[0, 0, :n_var[0, 0]] == 1).all()
    assert all(value_text(2, 1, *sl[0, 0, k].tolist()) == "NA" for k in range(n_var[0, 0]))
    assert n_var[0, 1] > 100 and sl[0, 1].max() > 1 and sl[0, 2].max() > 1
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_nsl_partial_last_word(gpu_lib, n, words):
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
def test_nsl_stride_edges(gpu_lib):
    """max_sites = the largest V; one less: that chain writes nothing and n_var stays; 0 with NULL members."""
    from popbam_amd import workload
    ctx, params, rows, types, flags = _shape("n12p2")
    n, masks = SHAPES["n12p2"]
    pop_n = [6, 6]
    wins = [(0, 4000), (100, 1100), (5, 5), (2000, 2300)]
    full, ms = _run_sized(ctx, rows, N_SITES, wins)
    n_var = full[0]
    assert ms == n_var.max() > 10
    _assert_same(full, ref_nsl(types, flags, masks, pop_n, wins, ms), "exact")
    less = _run_nsl(ctx, rows, N_SITES, wins, ms - 1)
    _assert_same(less, ref_nsl(types, flags, masks, pop_n, wins, ms - 1), "one less")
    big = np.argwhere(n_var == ms)
    assert len(big) >= 1
    for w, i in big.tolist():
        assert (less[1][w, i] == -1).all() and not less[3][w, i].any() and not less[4][w, i].any() and less[0][w, i] == ms
    small = np.argwhere((n_var < ms) & (n_var > 0))[0]
    assert less[3][small[0], small[1]].any()
    more = _run_nsl(ctx, rows, N_SITES, wins, ms + 70)   # unused slots past one stride of lanes
    _assert_same(more, ref_nsl(types, flags, masks, pop_n, wins, ms + 70), "more")
    # row and m alone: no walk
    part = workload.Nsl(ctx, len(wins), ms)
    part.sl.fill_(9)
    part.cens.fill_(9)
    part.out.sl = part.out.cens = None
    part(rows, _wins_tensor(wins), N_SITES)
    ctx.sync_check()
    got = _arrays(part, NAMES)
    assert all(np.array_equal(got[k], full[k]) for k in (0, 1, 2)) and (got[3] == 9).all() and (got[4] == 9).all()


@pytest.mark.gpu
def test_nsl_argument_errors(gpu_lib):
    from popbam_amd import _lib, workload
    ctx, params, rows, types, flags = _shape("n12p2")
    wins = _wins_tensor([(0, 1000)])
    j = workload.Nsl(ctx, 1, 64)
    lib, s = ctx.lib, workload.stream_handle()
    r, w, o, out = rows.data_ptr(), wins.data_ptr(), C.byref(j.opts), C.byref(j.out)
    assert lib.pbg_window_nsl(None, r, N_SITES, w, 1, o, out, s) == _lib.PBG_E_ARG
    for args in ((None, N_SITES, w, 1, o, out), (r, N_SITES, None, 1, o, out), (r, N_SITES, w, 1, None, out),
                 (r, N_SITES, w, 1, o, None)):
        assert lib.pbg_window_nsl(ctx.h, *args, s) == _lib.PBG_E_ARG
        assert lib.pbg_last_error(ctx.h)
    bad = _lib.PbgNslOpts(-1, 0)
    assert lib.pbg_window_nsl(ctx.h, r, N_SITES, w, 1, C.byref(bad), out, s) == _lib.PBG_E_ARG
    assert b"max_sites" in lib.pbg_last_error(ctx.h)
    zero = _lib.PbgNslOpts(0, 0)
    for nm in NAMES[1:]:   # a per-site member with no room for a site
        one = _lib.PbgNslOut(j.n_var.data_ptr(), None, None, None, None)
        setattr(one, nm, getattr(j, nm).data_ptr())
        assert lib.pbg_window_nsl(ctx.h, r, N_SITES, w, 1, C.byref(zero), C.byref(one), s) == _lib.PBG_E_ARG
        assert b"max_sites" in lib.pbg_last_error(ctx.h)
    for nm in ("sl", "cens"):   # the backward walk reads the sites back through row
        one = _lib.PbgNslOut(j.n_var.data_ptr(), None, j.m.data_ptr(), None, None)
        setattr(one, nm, getattr(j, nm).data_ptr())
        assert lib.pbg_window_nsl(ctx.h, r, N_SITES, w, 1, o, C.byref(one), s) == _lib.PBG_E_ARG
        assert b"row" in lib.pbg_last_error(ctx.h)
    # the count-only call with NULL per-site members, and no output at all
    for members in ((j.n_var.data_ptr(), None, None, None, None), (None,) * 5):
        assert lib.pbg_window_nsl(ctx.h, r, N_SITES, w, 1, C.byref(zero), C.byref(_lib.PbgNslOut(*members)), s) == _lib.PBG_OK
    # no window: PBG_OK, nothing written
    assert workload.Nsl(ctx, 0, 8).run(rows, wins, N_SITES) == _lib.PBG_OK
    ctx.sync_check()
    # pop_n that is not the masks' popcount
    p2 = _params(12, _blocks([6, 6]))
    p2.pop_n[1] = 5
    c2 = _lib.Context(p2, 0)
    j2 = workload.Nsl(c2, 1, 64)
    assert j2.run(rows, wins, N_SITES) == _lib.PBG_E_ARG and b"pop_n" in lib.pbg_last_error(c2.h)
    c2.close()
    # a window past the rows is never read: an empty window's outputs, reported by pbg_check
    over = workload.Nsl(ctx, 3, 64)
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
    assert 0 < j.n_var[0].min() and j.n_var[0].max() <= 64 and j.sl[0].max() > 0


@pytest.mark.gpu
def test_nsl_is_deterministic_and_interleaves_with_the_other_calls(gpu_lib):
    """Statistics, decay, nSL, joint spectrum, nSL, D statistics, the haplotype spectrum, Rmin, nSL,
    statistics, with the same pointers on one context and stream: each equals its own stand-alone run on
    a fresh context byte for byte, and two nSL runs give equal bytes."""
    from popbam_amd import workload
    T = [(0, 1, 2), (0, 2, 1), (1, 2, 0)]

    def others(wins):
        nw = len(wins)
        return {"jsfs": (lambda ctx: workload.JointSfs(ctx, nw), ("cells", "diffs", "fst")),
                "decay": (lambda ctx: workload.LdDecay(ctx, nw, 100, 100), ("pairs", "r2_sum", "n_var")),
                "dstat": (lambda ctx: workload.DStat(ctx, nw, T), ("sums", "d", "fd", "fdm")),
                "hfs": (lambda ctx: workload.Hfs(ctx, nw), workload.Hfs.NAMES),
                "rmin": (lambda ctx: workload.Rmin(ctx, nw, 1, 16), workload.Rmin.NAMES)}

    _interleaving("nsl", ("Nsl",), others, ("decay", "nsl", "jsfs", "nsl", "dstat", "hfs", "rmin", "nsl"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12p2", "n40p2i", "n126p3"])
def test_nsl_under_the_bounds_build(gpu_lib, tmp_path, name):
    """Called rows through the PBG_BOUNDS build (a fresh process): the same rows and the checker's numbers."""
    if not os.path.exists(BOUNDS_LIB):
        pytest.skip("the bounds build is not there (make bounds)")
    ctx, params, rows, types, flags = _shape(name)
    n, masks = SHAPES[name]
    wins = _windows(N_SITES, False)
    pop_n = [bin(m).count("1") for m in masks]
    ints, seg = row_ints(types), (np.asarray(flags) & SEG) > 0
    ms = max(len(variable_sites(ints, seg, pm, n_i, a, b)) for a, b in wins if a < b for pm, n_i in zip(masks, pop_n))
    (brows, got), = _bounds_child(tmp_path, [dict(call="Nsl", n=n, masks=masks, wins=wins, n_rows=N_SITES, max_sites=ms,
                                                  synth=(N_SITES, 10, SEED + n))])
    assert np.array_equal(brows, rows.cpu().numpy())
    _assert_same(got, ref_nsl(types, flags, masks, pop_n, wins, ms), "bounds")


# ---- command lines -----------------------------------------------------------------------
def _split_nsl(line, pops):
    """(the part before the nsl columns, {pop: [(pos, m, value text, c)]})."""
    at = line.index("\tnsl[")
    f = line[at + 1:].split("\t")
    assert len(f) == 2 * len(pops), f
    ext = {}
    for i, p in enumerate(pops):
        assert f[2 * i] == f"nsl[{p}]:", f
        toks = [] if f[2 * i + 1] == "NA" else [t.split(":") for t in f[2 * i + 1].split(",")]
        assert all(len(t) == 4 for t in toks), f
        ext[p] = [(int(a), int(b), v, int(c)) for a, b, v, c in toks]
    return line[:at], ext


def _check_text(ours, plain, pops, pop_n, res, pos0, what):
    """Every line: the plain line, then per population the checker's tokens."""
    n_var, row, m, sl, cens = res
    lines, plain_lines = ours.splitlines(), plain.splitlines()
    assert len(lines) == len(plain_lines) == len(n_var) > 0
    values = 0
    for w, (line, pl) in enumerate(zip(lines, plain_lines)):
        head, ext = _split_nsl(line, pops)
        assert head == pl, (what, w)
        for i, p in enumerate(pops):
            V = n_var[w, i]
            want = [(int(row[w, i, k]) + pos0 + 1, int(m[w, i, k]), value_text(pop_n[i], int(m[w, i, k]), *sl[w, i, k].tolist()),
                     int(cens[w, i, k].sum())) for k in range(V)]
            assert ext[p] == want, (what, w, p)
            values += sum(v != "NA" for _, _, v, _ in want)
    return values


CMD_CASES = [(nm, extra) for nm in ("g01_base", "g03_threepops") for extra in ((), ("-o", "1"), ("-o", "2"), ("--hfs",), ("-o", "1", "--hfs"))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,extra", CMD_CASES, ids=[nm + "".join(e).replace("-", "") for nm, e in CMD_CASES])
def test_nsl_command_line_on_a_golden_bam(gpu_lib, name, extra):
    """`popbam haplo -w 1 [-o N] [--hfs] --nsl` through cli.run and the native binary: the same text from
    both; the part before the nsl columns is the run without --nsl (the golden text where there is
    one); the tokens are the checker's on the stream's rows."""
    import torch
    from popbam_amd import _lib, engine, workload
    case = fixtures.load_case(name)
    d = case["dir"]
    args = ["haplo", "-w", "1"] + list(extra)
    base = ["haplo", "-f", os.path.join(d, "ref.fa"), "-w", "1"] + list(extra)
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run(base[0], base[1:] + tail)
    ours = cli.run(base[0], base[1:] + ["--nsl"] + tail)
    rc, nat, err = _native(base[:1] + ["--nsl"] + base[1:] + tail)   # the token in front here, at the end there
    assert rc == 0, err
    assert nat == ours
    gold = [c for c in case["meta"]["cases"] if c["args"] == args]
    assert bool(gold) == ("--hfs" not in extra)
    if gold:
        assert plain == fixtures.golden_text(name, gold[0]["stdout"])
    st = harness.Setup(name, args + ["--nsl"], "chr1")
    assert st.opts.nsl == 1 and st.opts.output == (int(extra[1]) if "-o" in extra else 0)
    ctx = _lib.Context(engine.make_params(st.opts, st.sm), 0)
    kb = st.kbatch
    ref = np.ascontiguousarray(kb["ref"], dtype=np.uint8)
    k = np.ascontiguousarray(kb["k"], dtype=np.uint8 if ctx.k_bytes == 1 else np.uint16)
    rq = np.ascontiguousarray(kb["rmsq"], dtype=np.uint32)
    keys = np.ascontiguousarray(kb["keys"], dtype=np.uint16)
    L = len(ref)
    cmd = engine._Cmd(st.opts, st.sm, st.chr, st.beg, st.end)
    assert cmd.c.output == st.opts.output | _lib.PBG_HAPLO_NSL
    rows = torch.zeros(L * ctx.row_bytes, dtype=torch.uint8, device="cuda")
    with _lib.Stream(ctx, [cmd.c], 0, L) as s:
        s.push(_lib.PbgPileup(L, 0, ref.ctypes.data, k.ctypes.data, rq.ctypes.data, None, keys.ctypes.data))
        s.finish()
        text = s.text(0)
        s.rows_into(rows.data_ptr(), rows.numel())
    assert text == ours
    wins = workload.reference_windows(st.beg, st.end, st.opts.win_size)
    types, flags = harness.rows_to_sites(rows.cpu().numpy(), ctx.row_bytes, L, st.sm.n)
    ms = max(1, max(len(variable_sites(row_ints(types), (flags & SEG) > 0, pm, n_i, a, b)) for a, b in wins
                    for pm, n_i in zip(st.masks, st.pop_n)))
    res = ref_nsl(types, flags, st.masks, st.pop_n, wins, ms)
    _assert_same(_run_nsl(ctx, rows, L, wins, ms), res, name)
    assert res[0].max() > 1
    _check_text(ours, plain, st.sm.pops, st.pop_n, res, 0, name)   # rows are contig positions here
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("output,hfs", [(0, 0), (1, 1), (2, 0)])
def test_nsl_on_a_synthetic_stream(gpu_lib, output, hfs):
    """A streamed run of `haplo -w 1000 [-o N] [--hfs] --nsl` over a synthetic batch of 24 samples in
    three populations: the line without its nsl columns is the stream's line without the bit, and the
    tokens are the checker's on the stream's rows (values that are numbers among them)."""
    import torch
    from popbam_amd import _lib, workload
    n, npops, L, W = 24, 3, 64 * 250, 1000
    ctx = _lib.Context(workload.default_params(n, npops), 0)
    syn = workload.SynthPileup(ctx, L, 10, SEED + 5)
    hp = workload.HotPath(ctx, syn, [(0, L)], 0)
    hp.call()
    ctx.sync_check()
    host = hp.to_host()
    keep = [b"chr1", (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)]), (C.c_char_p * npops)(*[f"p{i}".encode() for i in range(npops)])]

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
    ours, rows = run(output | _lib.PBG_HAPLO_NSL)
    assert torch.equal(rows, rows0) and torch.equal(rows, hp.rows)
    masks = [ctx.params.get_pop_mask(i) for i in range(npops)]
    pop_n = [ctx.params.pop_n[i] for i in range(npops)]
    wins = workload.reference_windows(0, L, W)
    types, flags = harness.rows_to_sites(rows.cpu().numpy(), ctx.row_bytes, L, n)
    got, ms = _run_sized(ctx, rows, L, wins)
    res = ref_nsl(types, flags, masks, pop_n, wins, ms)
    _assert_same(got, res, "stream")
    assert _check_text(ours, plain, [f"p{i}" for i in range(npops)], pop_n, res, 0, "stream") > 10
    ctx.close()
