"""nucdiv --snn (pbg_window_snn): the exact sample-by-sample difference matrix of a window and Hudson's
nearest-neighbour statistic Snn with its permutation test, per window and group of populations.

The reference has no such output, so the checker lives here: the contract of include/popbam_gpu.h restated
in numpy twice -- ref_snn_literal with loops over members and Python integers for the hash, ref_snn
vectorised with uint64 arithmetic and a stable sort for the ranks.  The two are compared with each other,
with the header's check vector and with a window derived by hand; the GPU results are compared with the
vectorised one.  Every comparison is exact: diff, near and ge as integers, snn bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fixtures
import harness
from window_helpers import _arrays, _blocks, _native, _wins_tensor, bits
from window_helpers import PARTIAL_WORD_CASES, partial_rows
from popbam_amd import cli
from popbam_amd import options as opt
from popbam_amd._lib import PBG_NUCDIV_SNN, PBG_SNN_MAX_PERMS   # the feature itself: absent, nothing here can run

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")
SEED = 0x4A1   # test_nsl.py's: the same called rows
COUNTED, SEG = 2, 4   # harness flags bits
NAMES = ("diff", "snn", "near", "ge")
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15


# ---- the checker -------------------------------------------------------------------------
def mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def perm_base(seed, K):
    return mix(((seed << 32) | (K & 0xFFFFFFFF)) & M64)


def perm_key(base, r, s):
    pr = mix((base + (r + 1) * G) & M64)
    return mix((pr + (s + 1) * G) & M64)


def literal_ranks(base, r, members):
    """rank of every member in the order by (key, sample id) ascending"""
    keyed = sorted((perm_key(base, r, s), s) for s in members)
    where = {s: k for k, (_, s) in enumerate(keyed)}
    return [where[s] for s in members]


def mix_np(z):
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def ranks_np(base, r0, r1, members):
    """[r1 - r0, N] ranks of permutations r0 .. r1 - 1, vectorised: uint64 wrap-around arithmetic and a
    stable sort (the members ascend, so equal keys fall in sample order)"""
    with np.errstate(over="ignore"):
        rr = np.arange(r0 + 1, r1 + 1, dtype=np.uint64)
        pr = mix_np(np.uint64(base) + rr * np.uint64(G))
        s1 = np.asarray(members, dtype=np.uint64) + np.uint64(1)
        keys = mix_np(pr[:, None] + s1[None, :] * np.uint64(G))
    order = np.argsort(keys, axis=1, kind="stable")
    ranks = np.empty_like(order)
    np.put_along_axis(ranks, order, np.broadcast_to(np.arange(order.shape[1]), order.shape), axis=1)
    return ranks


def sample_bits(types, n):
    """types ([L] u64 or [L, 2]) -> [L, n] 0/1"""
    types = np.asarray(types, dtype=np.uint64)
    if types.ndim == 1:
        types = types[:, None]
    cols = [(types[:, s >> 6] >> np.uint64(s & 63)) & np.uint64(1) for s in range(n)]
    return np.stack(cols, axis=1).astype(np.int64) if len(types) else np.zeros((0, n), np.int64)


def window_matrix(sb, seg, beg, end, n_rows):
    """the full symmetric [n, n] difference matrix of window [beg, end) over the segregating rows"""
    n = sb.shape[1]
    if not (end > beg and beg >= 0 and end <= n_rows):
        return np.zeros((n, n), np.int64)
    x = sb[beg:end][seg[beg:end]]
    return x.T @ (1 - x) + (1 - x).T @ x


def pair_list(n):
    return [(u, v) for u in range(n) for v in range(u + 1, n)]


def group_members(masks, group):
    """(sample ids ascending, their population) of a group of population indices"""
    mem = sorted((s, i) for i in group for s in range(128) if (masks[i] >> s) & 1)
    return [s for s, _ in mem], [i for _, i in mem]


def ordered_sum(S):
    """S: {t: S_t} -> the contract's sequential double sum in ascending t"""
    total = 0.0
    for t in sorted(S):
        total += float(S[t]) / float(t)
    return total


def snn_literal(D, members, labels, base, n_perms):
    """(snn, sum W, sum T, ge) of one group, with loops over members"""
    N = len(members)

    def stat(lab):
        S, sw, st = {}, 0, 0
        for a in range(N):
            ds = [D[members[a], members[b]] for b in range(N) if b != a]
            m = min(ds)
            nb = [b for b in range(N) if b != a and D[members[a], members[b]] == m]
            T, W = len(nb), sum(1 for b in nb if lab[b] == lab[a])
            S[T] = S.get(T, 0) + W
            sw, st = sw + W, st + T
        return ordered_sum(S), sw, st

    total, sw, st = stat(labels)
    ge = 0
    for r in range(n_perms):
        rk = literal_ranks(base, r, members)
        ge += stat([labels[k] for k in rk])[0] >= total
    return total / float(N), sw, st, ge


def snn_vector(D, members, labels, base, n_perms):
    N = len(members)
    sub = D[np.ix_(members, members)].astype(np.int64)
    off = ~np.eye(N, dtype=bool)
    m = np.where(off, sub, np.iinfo(np.int64).max).min(axis=1)
    NN = (sub == m[:, None]) & off
    T = NN.sum(axis=1)
    lab = np.asarray(labels)
    tvals = np.unique(T)

    def sums(pl):   # pl [R, N] -> [R] doubles, the sequential sum in ascending t
        W = (NN[None] & (pl[:, :, None] == pl[:, None, :])).sum(axis=2)
        total = np.zeros(len(pl), np.float64)
        for t in tvals:
            total = total + W[:, T == t].sum(axis=1).astype(np.float64) / np.float64(t)
        return total, W

    obs, W = sums(lab[None])
    ge = 0
    for r0 in range(0, n_perms, 256):   # bounded temporaries
        ge += int((sums(lab[ranks_np(base, r0, min(n_perms, r0 + 256), members)])[0] >= obs[0]).sum())
    return obs[0] / np.float64(N), int(W.sum()), int(T.sum()), ge


def ref_snn(types, flags, n, masks, wins, groups, n_perms, seed=0, key0=0, one=snn_vector):
    """(diff [n_win, n (n - 1) / 2] int32, snn [n_win, n_groups] f64, near [n_win, n_groups, 2] int32,
    ge [n_win, n_groups] int32) by the contract"""
    sb, seg = sample_bits(types, n), (np.asarray(flags) & SEG) > 0
    pl = pair_list(n)
    iu, iv = np.array([u for u, _ in pl], int), np.array([v for _, v in pl], int)
    nw, ng = len(wins), len(groups)
    diff = np.zeros((nw, len(pl)), np.int32)
    snn, near, ge = np.zeros((nw, ng)), np.zeros((nw, ng, 2), np.int32), np.zeros((nw, ng), np.int32)
    mem = [group_members(masks, g) for g in groups]
    for w, (beg, end) in enumerate(wins):
        D = window_matrix(sb, seg, beg, end, len(flags))
        if len(pl):
            diff[w] = D[iu, iv]
        base = perm_base(seed, (key0 + (beg & 0xFFFFFFFF)) & 0xFFFFFFFF)
        for e, (members, labels) in enumerate(mem):
            snn[w, e], near[w, e, 0], near[w, e, 1], ge[w, e] = one(D, members, labels, base, n_perms)
    return diff, snn, near, ge


def default_groups(np_):
    return ([tuple(range(np_))] if np_ >= 3 else []) + [(i, j) for i in range(np_) for j in range(i + 1, np_)]


def _assert_same(got, want, what=""):
    for k, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        same = np.array_equal(bits(g), bits(w)) if g.dtype == np.float64 else np.array_equal(g, w)
        assert same, (what, k, np.argwhere(np.asarray(g != w))[:5].tolist() if g.dtype != np.float64 else
                      np.argwhere(bits(g).reshape(g.shape) != bits(w).reshape(w.shape))[:5].tolist())


def _founder_types(rng, L, n, founders):
    """Rows in which every sample copies one of a few founders (the copy changes every 64 rows): samples
    on one founder are identical for the whole stretch, so nearest neighbours tie (test_nsl.py's)."""
    out = np.zeros((L, 2), np.uint64)
    for r0 in range(0, L, 64):
        src = rng.integers(0, founders, n)
        fb = rng.integers(0, 2, (min(64, L - r0), founders))
        sb = fb[:, src]   # [rows, n]
        for s in range(n):
            out[r0:r0 + len(sb), s >> 6] |= sb[:, s].astype(np.uint64) << np.uint64(s & 63)
    return out if n > 64 else out[:, 0].copy()


def _random_types(rng, L, n):
    t = np.zeros((L, 2), np.uint64)
    t[:, 0] = rng.integers(0, 1 << min(n, 64), L, dtype=np.uint64) if n < 64 else rng.integers(0, 1 << 64, L, dtype=np.uint64)
    if n > 64:
        t[:, 1] = rng.integers(0, 1 << (n - 64), L, dtype=np.uint64)
    return t if n > 64 else t[:, 0].copy()


# ---- CPU tests ---------------------------------------------------------------------------
CPU_CASES = [(6, [0b000111, 0b111000]), (9, [0b000000111, 0b000111000, 0b111000000]),
             (12, [0x555, 0xAAA]), (10, [0b0000000001, 0b0000011110, 0b1111100000]), (70, _blocks([30, 39, 1]))]


@pytest.mark.parametrize("n,masks", CPU_CASES, ids=[f"n{n}p{len(m)}" for n, m in CPU_CASES])
def test_the_two_restatements_agree(n, masks):
    rng = np.random.default_rng(n)
    L = 150
    groups = default_groups(len(masks))
    for kind in ("random", "founder", "founder2"):
        types = _random_types(rng, L, n) if kind == "random" else _founder_types(rng, L, n, 3 if kind == "founder" else 2)
        flags = np.where(rng.random(L) < 0.6, COUNTED | SEG, COUNTED).astype(np.uint8)
        wins = [(0, L), (10, 14), (64, 128), (7, 7), (30, 31)]
        perms = 12 if n > 12 else 40
        a = ref_snn(types, flags, n, masks, wins, groups, perms, 3, 1000, snn_literal)
        b = ref_snn(types, flags, n, masks, wins, groups, perms, 3, 1000, snn_vector)
        _assert_same(b, a, kind)
        assert a[0].max() > 0 and (a[3] <= perms).all()
    # the ranks themselves
    members = [s for s in range(n) if s % 3 != 1]
    base = perm_base(9, 77)
    assert ranks_np(base, 0, 20, members).tolist() == [literal_ranks(base, r, members) for r in range(20)]
    assert ranks_np(base, 5, 20, members).tolist() == [literal_ranks(base, r, members) for r in range(5, 20)]


def test_check_vector():
    """include/popbam_gpu.h's: seed 7, K 3, r 0, samples 0..11"""
    assert mix(1) == 0x5692161D100B05E5
    base = perm_base(7, 3)
    assert base == 0x50A440ECF5AB7340
    assert mix((base + G) & M64) == 0xBDFDE746D8CF90EC
    assert perm_key(base, 0, 0) == 0x0C22C8FE35277F90
    want = [1, 2, 9, 7, 3, 10, 8, 0, 11, 5, 4, 6]
    assert literal_ranks(base, 0, list(range(12))) == want == ranks_np(base, 0, 1, list(range(12)))[0].tolist()
    assert int(mix_np(np.array([1], np.uint64))[0]) == mix(1)


def test_ties_do_not_depend_on_the_labels():
    """T_a is the same under every permutation: it is a property of the distances alone"""
    rng = np.random.default_rng(5)
    n, masks = 12, [0x03F, 0xFC0]
    types = _founder_types(rng, 100, n, 3)
    D = window_matrix(sample_bits(types, n), np.ones(100, bool), 0, 100, 100)
    members, labels = group_members(masks, (0, 1))

    def ties(lab):
        out = []
        for a in range(n):
            m = min(D[a, b] for b in range(n) if b != a)
            out.append(sum(1 for b in range(n) if b != a and D[a, b] == m))
        return out

    t0 = ties(labels)
    assert max(t0) > 1
    base = perm_base(0, 0)
    for r in range(50):
        assert ties([labels[k] for k in literal_ranks(base, r, members)]) == t0
    # and near[1] of the checker is their sum whatever the seed
    for seed in (0, 1, 2):
        assert snn_vector(D, members, labels, perm_base(seed, 0), 5)[2] == sum(t0)


# six samples, populations {0, 1, 2} and {3, 4, 5}; row r's bit s = sample s carries the derived allele.
#   sample:  0 1 2 3 4 5
#   row 0    . 1 1 . . 1
#   row 1    . . 1 . . .
#   row 2,3  . . . 1 1 1
#   row 4,5  . . . 1 1 .
#   row 6    . . . . 1 .
#   row 7    1 1 1 . . .   not segregating: never counted
HAND_TYPES = np.array([0b100110, 0b000100, 0b111000, 0b111000, 0b011000, 0b011000, 0b010000, 0b000111], np.uint64)
HAND_FLAGS = np.array([COUNTED | SEG] * 7 + [COUNTED], np.uint8)
HAND_MASKS = [0b000111, 0b111000]
HAND_WINS = [(0, 8), (2, 6), (7, 8), (3, 3)]
# window (0, 8): d01 = 1, d02 = 2, d03 = 4, d04 = 5, d05 = 3, d12 = 1, d13 = 5, d14 = 6, d15 = 2, d23 = 6,
# d24 = 7, d25 = 3, d34 = 1, d35 = 3, d45 = 4.  Nearest: 0 -> {1}; 1 -> {0, 2}; 2 -> {1}; 3 -> {4}; 4 -> {3};
# 5 -> {1} (distance 2, the other population).  T = 1 2 1 1 1 1, W = 1 2 1 1 1 0: S_1 = 4, S_2 = 2,
# sum = 4 / 1 + 2 / 2 = 5, snn = 5 / 6.
# window (2, 6): samples 0, 1, 2 are identical (0000), 3 and 4 identical (1111), 5 is 1100, at distance 2
# from everyone.  T = 2 2 2 1 1 5, W = 2 2 2 1 1 2: S_1 = 2, S_2 = 6, S_5 = 2, sum = 2 + 3 + 2 / 5.
# window (7, 8) has no segregating row, (3, 3) no row: every member ties with the five others, W = 2 each,
# S_5 = 12, sum = 12 / 5, snn = (3 * 2 + 3 * 2) / (6 * 5) by the same arithmetic.
HAND_DIFF0 = [1, 2, 4, 5, 3, 1, 5, 6, 2, 6, 7, 3, 1, 3, 4]
HAND_DIFF1 = [0, 0, 4, 4, 2, 0, 4, 4, 2, 4, 4, 2, 0, 2, 2]
HAND_SNN = [(4.0 / 1.0 + 2.0 / 2.0) / 6.0, ((2.0 / 1.0 + 6.0 / 2.0) + 2.0 / 5.0) / 6.0, (12.0 / 5.0) / 6.0, (12.0 / 5.0) / 6.0]
HAND_NEAR = [(6, 7), (10, 13), (12, 30), (12, 30)]


def _hand_made_expectations(diff, snn, near, ge, n_perms):
    assert diff[0].tolist() == HAND_DIFF0 and diff[1].tolist() == HAND_DIFF1 and not diff[2:].any()
    assert bits(snn[:, 0]).tolist() == bits(np.array(HAND_SNN)).tolist()
    assert near[:, 0].tolist() == [list(x) for x in HAND_NEAR]
    assert ge[2:, 0].tolist() == [n_perms, n_perms] and (ge <= n_perms).all()


def test_checker_on_a_hand_made_window():
    for one in (snn_literal, snn_vector):
        for perms in (0, 30):
            _hand_made_expectations(*ref_snn(HAND_TYPES, HAND_FLAGS, 6, HAND_MASKS, HAND_WINS, [(0, 1)], perms, 0, 0, one), perms)


def _separated(L=40):
    """two populations of six, every row fixed between them"""
    return np.full(L, 0b111111000000, np.uint64), np.full(L, COUNTED | SEG, np.uint8), [0x03F, 0xFC0]


def _keep_or_swap(seed, K, n_perms):
    """the permutations that leave the partition {0..5}, {6..11} as it is, counted from the ranks"""
    base, cnt = perm_base(seed, K), 0
    for r in range(n_perms):
        side = [k // 6 for k in literal_ranks(base, r, list(range(12)))]
        cnt += len(set(side[:6])) == 1 and len(set(side[6:])) == 1
    return cnt


def test_two_separated_populations_give_one():
    types, flags, masks = _separated()
    for seed, perms in ((0, 1000), (11, 300)):
        diff, snn, near, ge = ref_snn(types, flags, 12, masks, [(0, 40)], [(0, 1)], perms, seed, 17)
        assert snn[0, 0] == 1.0 and near[0].tolist() == [[60, 60]] and set(diff[0].tolist()) == {0, 40}
        assert ge[0, 0] == _keep_or_swap(seed, 17, perms)


def test_the_permutation_is_uniform_enough():
    """seed 1, K 5, 12 samples, r = 0 .. 11,999: with twelve distinct labels the label that lands on sample 0
    is the rank of sample 0.  Each value 850 to 1,150 times (a prototype gave 951 to 1,044); the draw is
    deterministic, so this cannot flake."""
    rk = np.concatenate([ranks_np(perm_base(1, 5), r0, r0 + 1000, list(range(12))) for r0 in range(0, 12000, 1000)])
    counts = np.bincount(rk[:, 0], minlength=12)
    print(counts.tolist())
    assert counts.sum() == 12000 and counts.min() >= 850 and counts.max() <= 1150
    assert sorted(rk[0].tolist()) == list(range(12))


def test_snn_option_parses():
    base = ["-f", "ref.fa", "-w", "10"]
    tail = ["in.bam", "chr1:1-500"]
    plain = opt.parse_args("nucdiv", base + tail)
    assert (plain.snn, plain.snn_perms, plain.snn_seed) == (0, 0, 0)
    for tok, want in (("--snn", (1000, 0)), ("--snn=0", (0, 0)), ("--snn=200,3", (200, 3)), ("--snn=65535,16383", (PBG_SNN_MAX_PERMS, opt.SNN_MAX_SEED)),
                      ("--snn=5", (5, 0)), ("--snn=007,01", (7, 1))):
        for argv in ([tok] + base + tail, base + [tok] + tail, base + tail + [tok]):
            o = opt.parse_args("nucdiv", argv)
            assert (o.snn, o.snn_perms, o.snn_seed) == (1,) + want, argv
            o.snn = o.snn_perms = o.snn_seed = 0
            assert o == plain   # every other field as without the token
    for bad in ("--snn=", "--snn=65536", "--snn=10,16384", "--snn=1,2,3", "--snn=-1", "--snn=+1", "--snn=1,", "--snn=,1",
                "--snn=1e2", "--snn= 1", "--snn=0x10", "--snn=99999999999999999999"):
        with pytest.raises(opt.PopbamError, match="Not a valid snn option"):
            opt.parse_args("nucdiv", base + [bad] + tail)
    # only nucdiv has it
    for cmd in ("haplo", "sfs", "ld", "diverge", "snp", "tree"):
        assert opt.parse_args(cmd, base + ["--snn=5,1"] + tail).snn == 0


def test_native_snn_errors_match_the_python_cli(capsys):
    d = fixtures.load_case("g01_base")["dir"]
    ref, bam = os.path.join(d, "ref.fa"), os.path.join(d, "in.bam")
    for tok in ("--snn=", "--snn=65536", "--snn=10,16384", "--snn=1,2,3", "--snn=-1", "--snn=1,", "--snn=x"):
        argv = ["nucdiv", "-f", ref, tok, bam, "chr1"]
        rc, out, err = _native(argv)
        prc = cli.main(argv)
        pe = capsys.readouterr()
        assert rc == prc == 1 and out == "" == pe.out, argv
        assert err == pe.err and "Not a valid snn option" in err, (argv, err, pe.err)


def test_snn_is_exported():
    from popbam_amd import _lib, workload
    assert "pbg_window_snn" in _lib.EXPORTS and hasattr(workload, "Snn")
    # bits of pbg_cmd.output, no new field: a program compiled against the header before it keeps running
    assert _lib.PBG_NUCDIV_SNN == 1 and ("hfs", C.c_int32) == _lib.PbgCmd._fields_[-1]
    assert (_lib.PBG_SNN_MAX_GROUPS, _lib.PBG_SNN_MAX_PERMS) == (4096, 65535)
    assert C.sizeof(_lib.PbgSnnOpts) == 24 and C.sizeof(_lib.PbgSnnOut) == 32
    assert [f for f, _ in _lib.PbgSnnOut._fields_] == list(NAMES)
    assert workload.Snn.default_groups(1) == [] and workload.Snn.default_groups(2) == [(0, 1)]
    assert workload.Snn.default_groups(3) == [(0, 1, 2), (0, 1), (0, 2), (1, 2)] == default_groups(3)


# ---- GPU tests ---------------------------------------------------------------------------
N_SITES = 32_000
SHAPES = {   # name -> (samples, population masks, permutations)
    "n12p2": (12, _blocks([6, 6]), 1000),                             # 2-byte rows
    "n24p3": (24, _blocks([8, 8, 8]), 200),                           # 4-byte rows
    "n40p2i": (40, [sum(1 << s for s in range(0, 40, 2)), sum(1 << s for s in range(1, 40, 2))], 200),   # 8-byte rows
    "n126p3": (126, _blocks([70, 50, 6]), 100),                       # 16-byte rows; groups of 126, 120, 76 and 56
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
        n, masks, _ = SHAPES[name]
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


def _windows(n_sites, few=False):
    """Windows from 3 rows up: overlapping, the whole batch, empty, beg == end, beg > end."""
    rng = np.random.default_rng(7)
    wins = [(0, n_sites), (0, 2_000), (9_999, 12_001), (5, 5), (0, 1), (9, 4)]
    for ln in ((30, 1000) if few else (3, 10, 30, 60, 100, 300, 1000, 3000)):
        for s in rng.integers(0, n_sites - ln, 1 if few else 2):
            wins.append((int(s), int(s) + ln))
    return wins


def _run_snn(ctx, rows, n_rows, wins, groups=(), n_perms=0, seed=0, key0=0, check=True):
    from popbam_amd import workload
    j = workload.Snn(ctx, len(wins), groups, n_perms, seed, key0)
    j(rows, _wins_tensor(wins), n_rows)
    if check:
        ctx.sync_check()
    return _arrays(j, NAMES)


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


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SHAPES))
def test_snn_matches_the_checker_on_called_rows(gpu_lib, name):
    ctx, params, rows, types, flags = _shape(name)
    n, masks, perms = SHAPES[name]
    wins = _windows(N_SITES, few=n > 64)
    groups = default_groups(len(masks))
    got = _run_snn(ctx, rows, N_SITES, wins, groups, perms, 5, 1234)
    _assert_same(got, ref_snn(types, flags, n, masks, wins, groups, perms, 5, 1234), name)
    diff, snn, near, ge = got
    assert diff[0].max() > 100 and not diff[[3, 5]].any() and (ge[[3, 5]] == perms).all()
    assert ((ge > 0) & (ge < perms)).any() and (near[..., 1] >= near[..., 0]).all()


@pytest.mark.gpu
def test_snn_on_the_hand_made_window(gpu_lib):
    ctx, params, rows = _crafted(6, HAND_MASKS, HAND_TYPES, HAND_FLAGS)
    for perms in (0, 30):
        got = _run_snn(ctx, rows, len(HAND_FLAGS), HAND_WINS, [(0, 1)], perms)
        _hand_made_expectations(*got, perms)
        _assert_same(got, ref_snn(HAND_TYPES, HAND_FLAGS, 6, HAND_MASKS, HAND_WINS, [(0, 1)], perms))
    ctx.close()


@pytest.mark.gpu
def test_snn_of_two_separated_populations(gpu_lib):
    types, flags, masks = _separated()
    ctx, params, rows = _crafted(12, masks, types, flags)
    diff, snn, near, ge = _run_snn(ctx, rows, 40, [(0, 40)], [(0, 1)], 1000, 0, 17)
    assert snn[0, 0] == 1.0 and ge[0, 0] == _keep_or_swap(0, 17, 1000) and near[0].tolist() == [[60, 60]]
    ctx.close()


# groups of N members on founder rows: N' = 2, 4, 16, 32, 64 and the two-members-a-lane path at its edges;
# populations of one sample (W = 0 always) and interleaved masks
def _lane_case(N):
    if N == 2:
        return 3, [0b001, 0b100], 2           # two populations of one sample; sample 1 in none
    if N == 3:
        return 5, [0b00001, 0b10100], 2
    if N in (16, 17):
        return N + 1, [sum(1 << s for s in range(0, N, 2)), sum(1 << s for s in range(1, N, 2)), 1 << N], 3   # interleaved
    if N in (32, 33):
        return N + 2, [(1 << 20) - 1, ((1 << N) - 1) ^ ((1 << 20) - 1) ^ (1 << 25), 1 << 25, 3 << N], 3   # a population of one inside
    if N in (64, 65):
        return N + 3, [sum(1 << s for s in range(0, N, 3)), sum(1 << s for s in range(1, N, 3)),
                       sum(1 << s for s in range(2, N, 3)), 7 << N], 3
    return 126, _blocks([63, 62, 1]), 4


LANE_N = [2, 3, 16, 17, 32, 33, 64, 65, 126]


@pytest.mark.gpu
@pytest.mark.parametrize("N", LANE_N)
def test_snn_lane_packing_edges(gpu_lib, N):
    n, masks, founders = _lane_case(N)
    rng = np.random.default_rng(N)
    L = 700
    types = _founder_types(rng, L, n, founders)
    flags = np.where(rng.random(L) < 0.7, COUNTED | SEG, COUNTED).astype(np.uint8)
    np_ = len(masks)
    first = (0, 1) if N <= 17 else (0, 1, 2)
    groups = [first] + [g for g in default_groups(np_) if len(g) == 2 and g != first][:3]
    assert len(group_members(masks, first)[0]) == N
    wins = [(0, L), (0, 64), (100, 130), (640, 700), (300, 300)]
    perms = 150 if N > 64 else 257
    ctx, params, rows = _crafted(n, masks, types, flags)
    got = _run_snn(ctx, rows, L, wins, groups, perms, 2, 9)
    _assert_same(got, ref_snn(types, flags, n, masks, wins, groups, perms, 2, 9), str(N))
    if N > 3:   # ties are there: some member has more than one nearest neighbour
        assert (got[2][..., 1] > [len(group_members(masks, g)[0]) for g in groups]).any()
    ctx.close()


@pytest.mark.gpu
def test_snn_permutation_count_edges(gpu_lib):
    from popbam_amd import workload
    ctx, params, rows, types, flags = _shape("n12p2")
    n, masks, _ = SHAPES["n12p2"]
    wins = [(100, 400), (5, 5), (2_000, 2_060)]
    many = False
    for perms in (0, 1, 3, 4, 5, 63, 64, 65, 1000):
        j = workload.Snn(ctx, len(wins), [(0, 1)], perms, 1, 0)
        chunks = j.chunks
        per = -(-perms // chunks) if perms else 0
        many |= chunks > 1 and perms % per != 0   # a last chunk that is shorter than the others
        got = _run_snn(ctx, rows, N_SITES, wins, [(0, 1)], perms, 1, 0)
        _assert_same(got, ref_snn(types, flags, n, masks, wins, [(0, 1)], perms, 1, 0), str(perms))
        assert (got[3][1] == perms).all()
    assert many
    assert workload.Snn(ctx, 1, [(0, 1)], 1000).chunks == 63 and workload.Snn(ctx, 5000, [(0, 1)], 1000).chunks == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n,founders", [(12, 3), (12, 4), (30, 3), (96, 4)], ids=["12f3", "12f4", "30f3", "96f4"])
def test_snn_ties(gpu_lib, n, founders):
    """3 to 4 founder haplotypes, duplicated samples, and a window with no segregating row"""
    rng = np.random.default_rng(n + founders)
    L = 400
    types = _founder_types(rng, L, n, founders)
    # samples 1 and n - 1 are copies of sample 0 everywhere
    t2 = types.reshape(L, -1).copy()
    for s in (1, n - 1):
        b0 = t2[:, 0] & np.uint64(1)
        t2[:, s >> 6] = (t2[:, s >> 6] & ~(np.uint64(1) << np.uint64(s & 63))) | (b0 << np.uint64(s & 63))
    types = t2 if n > 64 else t2[:, 0].copy()
    flags = np.where(rng.random(L) < 0.6, COUNTED | SEG, COUNTED).astype(np.uint8)
    flags[200:260] = COUNTED   # no segregating row in (200, 260)
    masks = _blocks([n // 2, n - n // 2]) if n < 90 else _blocks([40, 30, 26])
    groups = default_groups(len(masks))
    wins = [(0, L), (200, 260), (0, 64), (64, 128), (190, 270)]
    perms = 100 if n > 64 else 200
    ctx, params, rows = _crafted(n, masks, types, flags)
    got = _run_snn(ctx, rows, L, wins, groups, perms, 4, 50)
    _assert_same(got, ref_snn(types, flags, n, masks, wins, groups, perms, 4, 50))
    diff, snn, near, ge = got
    pl = pair_list(n)
    assert not diff[:, pl.index((0, 1))].any() and not diff[:, pl.index((0, n - 1))].any() and not diff[1].any()
    for e, g in enumerate(groups):   # the closed form
        sizes = [bin(masks[i]).count("1") for i in g]
        N = sum(sizes)
        assert ge[1, e] == perms and near[1, e].tolist() == [sum(s * (s - 1) for s in sizes), N * (N - 1)]
        assert snn[1, e] == (float(sum(s * (s - 1) for s in sizes)) / float(N - 1)) / float(N)
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 12])
def test_snn_has_no_16_bit_wrap(gpu_lib, n):
    """a window of 65,537 segregating rows with a sample pair that differs at all of them, beside tiny ones"""
    L = 65_537 + 40
    types = np.zeros(L, np.uint64)
    types[:65_537] = 0b0001          # sample 0 against every other
    types[0:65_537:2] |= 0b0100      # sample 2 at every other row
    types[65_537:] = np.arange(40, dtype=np.uint64) % np.uint64(1 << n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    masks = _blocks([n // 2, n // 2])
    wins = [(65_530, 65_545), (0, 65_537), (65_537, L), (3, 5)]
    ctx, params, rows = _crafted(n, masks, types, flags)
    got = _run_snn(ctx, rows, L, wins, [(0, 1)], 20, 0, 0)
    _assert_same(got, ref_snn(types, flags, n, masks, wins, [(0, 1)], 20, 0, 0))
    pl = pair_list(n)
    assert got[0][1, pl.index((0, 1))] == 65_537 and got[0][1, pl.index((0, 2))] == 32_768
    assert got[0][1, pl.index((1, 2))] == 32_769 and got[0][1].max() == 65_537
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12p2", "n24p3", "n126p3"])
def test_snn_differences_add_up_to_the_joint_spectrum_sums(gpu_lib, name):
    """for every population pair: the sum of diff over the within-population sample pairs is pbg_window_jsfs's
    SW_i and SW_j, over the between-population pairs its SB (int64, exact)"""
    from popbam_amd import workload
    ctx, params, rows, types, flags = _shape(name)
    n, masks, _ = SHAPES[name]
    wins = _windows(N_SITES)
    diff = _run_snn(ctx, rows, N_SITES, wins)[0].astype(np.int64)
    js = workload.JointSfs(ctx, len(wins), 0)   # no outgroup flip changes a pairwise difference
    js(rows, _wins_tensor(wins), N_SITES)
    ctx.sync_check()
    sums = js.diffs.cpu().numpy()
    pl = pair_list(n)
    popof = {s: i for i, m in enumerate(masks) for s in range(n) if (m >> s) & 1}
    pu, pv = np.array([popof[u] for u, _ in pl]), np.array([popof[v] for _, v in pl])
    p = 0
    for i in range(len(masks)):
        for j in range(i + 1, len(masks)):
            sw_i, sw_j = diff[:, (pu == i) & (pv == i)].sum(axis=1), diff[:, (pu == j) & (pv == j)].sum(axis=1)
            sb = diff[:, ((pu == i) & (pv == j)) | ((pu == j) & (pv == i))].sum(axis=1)
            assert np.array_equal(sums[:, p, 0], sw_i) and np.array_equal(sums[:, p, 1], sw_j), (name, i, j)
            assert np.array_equal(sums[:, p, 2], sb) and sb.max() > 0, (name, i, j)
            p += 1


@pytest.mark.gpu
@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_snn_partial_last_word(gpu_lib, n, words):
    """the batch ends inside a 16-byte word of rows, in a buffer of 0xFF bytes: nothing past the last row
    is counted"""
    L, extra = partial_rows(n, words)
    rng = np.random.default_rng(n)
    types = _random_types(rng, L, n)
    flags = np.full(L, COUNTED | SEG, np.uint8)
    masks = _blocks([n // 2, n // 2])
    ctx, params, rows = _crafted(n, masks, types, flags)
    wins = [(0, L), (L - 3, L), (L - 1, L), (L - 70, L)] + extra
    perms = 20 if n > 64 else 40
    got = _run_snn(ctx, _padded(rows), L, wins, [(0, 1)], perms, 1, 2)
    _assert_same(got, ref_snn(types, flags, n, masks, wins, [(0, 1)], perms, 1, 2))
    ctx.close()


@pytest.mark.gpu
def test_snn_window_and_argument_edges(gpu_lib):
    import torch
    from popbam_amd import _lib, workload
    ctx, params, rows, types, flags = _shape("n12p2")
    n, masks, _ = SHAPES["n12p2"]
    # beg >= end: zeros, and no range bit
    got = _run_snn(ctx, rows, N_SITES, [(7, 7), (9, 2), (100, 1_100)], [(0, 1)], 10)
    assert not got[0][:2].any() and (got[3][:2] == 10).all() and got[0][2].any()
    # a window outside the rows: not read, zeros, the range bit
    for bad in ((-1, 5), (N_SITES - 1, N_SITES + 1), (N_SITES + 5, N_SITES + 9)):
        j = workload.Snn(ctx, 2, [(0, 1)], 10)
        j.diff.fill_(-1)
        j(rows, _wins_tensor([bad, (100, 1_100)]), N_SITES)
        assert ctx.lib.pbg_check(ctx.h, None) == _lib.PBG_E_RANGE
        d, s, nr, ge = _arrays(j, NAMES)
        assert not d[0].any() and ge[0, 0] == 10 and np.array_equal(d[1], got[0][2]) and ge[1, 0] == got[3][2, 0]
    ctx.sync_check()
    # n_groups = 0 with one population: the difference matrix alone
    one = _lib.Context(_params(n, [(1 << n) - 1]), 0)
    d1 = _run_snn(one, rows, N_SITES, [(100, 1_100)])[0]
    assert np.array_equal(d1[0], got[0][2])
    wt = _wins_tensor([(100, 1_100)])
    j = workload.Snn(one, 1, [(0, 1)], 10)
    assert j.run(rows, wt, N_SITES) == _lib.PBG_E_ARG   # population 1 is not there
    one.close()

    def rc_of(gr=((0, 1),), perms=10, **kw):
        j = workload.Snn(ctx, 1, gr, perms)
        for k, v in kw.items():
            setattr(j.opts, k, v)
        return j.run(rows, wt, N_SITES)

    assert rc_of() == _lib.PBG_OK
    assert rc_of(n_groups=-1) == _lib.PBG_E_ARG and rc_of(n_groups=_lib.PBG_SNN_MAX_GROUPS + 1) == _lib.PBG_E_ARG
    assert rc_of(n_perms=-1) == _lib.PBG_E_ARG and rc_of(n_perms=_lib.PBG_SNN_MAX_PERMS + 1) == _lib.PBG_E_ARG
    assert rc_of(gr=((0,),)) == _lib.PBG_E_ARG          # fewer than two populations
    assert rc_of(gr=((0, 1), (1,))) == _lib.PBG_E_ARG
    assert rc_of(gr=((0, 2),)) == _lib.PBG_E_ARG        # a bit at n_pops
    assert rc_of(gr=((0, 1, 63),)) == _lib.PBG_E_ARG
    assert rc_of(groups=C.POINTER(C.c_uint64)()) == _lib.PBG_E_ARG   # NULL with n_groups > 0
    assert "snn" in ctx.lib.pbg_last_error(ctx.h).decode()
    j = workload.Snn(ctx, 1, [(0, 1)], 10)
    lib, h, st = ctx.lib, ctx.h, None
    ok = (h, rows.data_ptr(), N_SITES, wt.data_ptr(), 1, C.byref(j.opts), C.byref(j.out), st)
    for k in (0, 1, 3, 5, 6):
        a = list(ok)
        a[k] = None
        assert lib.pbg_window_snn(*a) == _lib.PBG_E_ARG, k
    a = list(ok)
    a[4] = 0
    assert lib.pbg_window_snn(*a) == _lib.PBG_OK   # n_win == 0
    ctx.sync_check()
    # each NULL output member: the others are as in the full call
    full = _run_snn(ctx, rows, N_SITES, [(100, 1_100)], [(0, 1)], 10)
    for k, nm in enumerate(NAMES):
        j = workload.Snn(ctx, 1, [(0, 1)], 10)
        getattr(j, nm).fill_(77)
        setattr(j.out, nm, None)
        j(rows, wt, N_SITES)
        ctx.sync_check()
        for k2, nm2 in enumerate(NAMES):
            g = getattr(j, nm2).cpu().numpy()
            assert (g == 77).all() if k2 == k else np.array_equal(bits(g) if k2 == 1 else g, bits(full[k2]) if k2 == 1 else full[k2]), (nm, nm2)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_snn_does_not_depend_on_the_place_in_the_list(gpu_lib):
    ctx, params, rows, types, flags = _shape("n24p3")
    n, masks, _ = SHAPES["n24p3"]
    wins = _windows(N_SITES)[1:]
    groups = default_groups(3)
    whole = _run_snn(ctx, rows, N_SITES, wins, groups, 100, 3, 500)
    h = len(wins) // 2
    a, b = _run_snn(ctx, rows, N_SITES, wins[:h], groups, 100, 3, 500), _run_snn(ctx, rows, N_SITES, wins[h:], groups, 100, 3, 500)
    _assert_same(tuple(np.concatenate([x, y]) for x, y in zip(a, b)), whole, "halves")
    # the rows shifted by 64 and key0 lowered by 64: key0 + beg is what counts
    rb = ctx.row_bytes
    keep = [(x, y) for x, y in wins if y <= x or x >= 64]
    shifted = rows[64 * rb:]
    got = _run_snn(ctx, shifted, N_SITES - 64, [(x - 64, y - 64) if y > x else (x, y) for x, y in keep], groups, 100, 3, 500 + 64)
    want = _run_snn(ctx, rows, N_SITES, keep, groups, 100, 3, 500)
    live = [k for k, (x, y) in enumerate(keep) if y > x]
    _assert_same(tuple(g[live] for g in got), tuple(w[live] for w in want), "shifted")
    # and the reversed list
    rev = _run_snn(ctx, rows, N_SITES, wins[::-1], groups, 100, 3, 500)
    _assert_same(tuple(g[::-1].copy() for g in rev), whole, "reversed")


@pytest.mark.gpu
def test_snn_is_deterministic_and_interleaves_with_the_other_calls(gpu_lib):
    """Statistics, Snn, joint spectrum, Snn (other options), nSL, Snn, statistics, with the same pointers on
    one context and stream: each equals its own stand-alone run on a fresh context byte for byte, and two
    Snn runs give equal bytes."""
    from popbam_amd import _lib, workload
    n, npops, L = 12, 3, 64 * 300
    wins = [(0, 6000)] + workload.reference_windows(0, L, 5_000) + [(s, s + 400) for s in range(0, 6000, 300)]
    groups = default_groups(npops)

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

    names_of = {"jsfs": ("cells", "diffs", "fst"), "nsl": workload.Nsl.NAMES, "snn": NAMES, "snn2": NAMES}
    make = {"jsfs": lambda ctx: workload.JointSfs(ctx, len(wins), 0), "nsl": lambda ctx: workload.Nsl(ctx, len(wins), 0),
            "snn": lambda ctx: workload.Snn(ctx, len(wins), groups, 100, 1, 2),
            "snn2": lambda ctx: workload.Snn(ctx, len(wins), groups[1:3], 37, 9, 2)}
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
    assert alone["snn"][0].max() > 0 and ((alone["snn"][3] > 0) & (alone["snn"][3] < 100)).any()

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    first = zns_out(hp)
    order = ("snn", "jsfs", "snn2", "nsl", "snn")
    ran = [(key, make[key](ctx)(hp.rows, hp.wins, L)) for key in order]
    zns(hp)
    ctx.sync_check()
    assert first == alone["zns"] == zns_out(hp)
    for key, x in ran:
        for g, w_, nm in zip(_arrays(x, names_of[key]), alone[key], names_of[key]):
            assert g.tobytes() == w_.tobytes(), (key, nm)
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
j = workload.Snn.of(hp, {groups!r}, {perms}, 5, 1234)
ctx.sync_check()   # raises when the error word is not 0
np.savez({out!r}, rows=hp.rows.cpu().numpy(), **{{k: getattr(j, k).cpu().numpy() for k in workload.Snn.NAMES}})
ctx.close()
print("ok")
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["n12p2", "n40p2i", "n126p3"])
def test_snn_under_the_bounds_build(gpu_lib, tmp_path, name):
    """Called rows through the PBG_BOUNDS build (a fresh process): the same rows and the checker's numbers,
    and the error word stays 0."""
    assert os.path.exists(BOUNDS_LIB), "the bounds build is not there: the Makefile's `bounds` target builds it"
    ctx, params, rows, types, flags = _shape(name)
    n, masks, perms = SHAPES[name]
    perms = min(perms, 100)
    out = str(tmp_path / "bounds.npz")
    env = dict(os.environ, POPBAM_GPU_LIB=BOUNDS_LIB)
    wins = _windows(N_SITES, few=True)
    groups = default_groups(len(masks))
    r = subprocess.run([sys.executable, "-c", BOUNDS_SNIPPET.format(repo=REPO, n=n, npops=len(masks), masks=masks, n_sites=N_SITES,
                                                                   seed=SEED + n, out=out, wins=wins, groups=groups, perms=perms)],
                       env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    z = np.load(out)
    assert np.array_equal(z["rows"], rows.cpu().numpy())
    _assert_same(tuple(z[k] for k in NAMES), ref_snn(types, flags, n, masks, wins, groups, perms, 5, 1234), "bounds")


# ---- command lines -----------------------------------------------------------------------
NA = "     NA"   # a column's NA as print_nucdiv writes it (setw(7))


def _group_names(pops):
    np_ = len(pops)
    return (["*"] if np_ >= 3 else []) + [f"{pops[i]},{pops[j]}" for i in range(np_) for j in range(i + 1, np_)]


def _want_text(plain, pops, perms, seg_rows, snn, ge):
    """every plain line with the columns the checker's numbers give"""
    out = []
    lines = plain.splitlines()
    assert len(lines) == len(snn) > 0
    for w, line in enumerate(lines):
        for e, nm in enumerate(_group_names(pops)):
            v = "%.5f" % snn[w, e] if seg_rows[w] else NA
            p = "%.5f" % (float(ge[w, e] + 1) / float(perms + 1)) if seg_rows[w] and perms else NA
            line += f"\tsnn[{nm}]:\t{v}\tpsnn[{nm}]:\t{p}"
        out.append(line + "\n")
    return "".join(out)


CMD_CASES = [("g01_base", "--snn=200,3"), ("g03_threepops", "--snn=200,3"), ("g03_threepops", "--snn=0"), ("g01_base", "--snn")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,tok", CMD_CASES, ids=[f"{nm}{t}".replace("--", "-").replace("=", "").replace(",", "_") for nm, t in CMD_CASES])
def test_snn_command_line_on_a_golden_bam(gpu_lib, name, tok, monkeypatch):
    """`popbam nucdiv -w 1 --snn[=PERMS[,SEED]]` through cli.run and the native binary: the same text from
    both, equal to the run without the token (the golden text where there is one) with the columns appended
    that the checker computes from the stream's rows; the same again in blocks of two windows; PERMS = 0
    prints NA for psnn."""
    import torch
    from popbam_amd import _lib, engine, workload
    case = fixtures.load_case(name)
    d = case["dir"]
    args = ["nucdiv", "-w", "1"]
    base = ["nucdiv", "-f", os.path.join(d, "ref.fa"), "-w", "1"]
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run(base[0], base[1:] + tail)
    ours = cli.run(base[0], base[1:] + [tok] + tail)
    rc, nat, err = _native(base[:1] + [tok] + base[1:] + tail)   # the token in front here, at the end there
    assert rc == 0, err
    assert nat == ours
    rc, nat_plain, err = _native(base + tail)
    assert rc == 0 and nat_plain == plain, err
    gold = [c for c in case["meta"]["cases"] if c["args"] == args]
    if gold:   # plain nucdiv is byte-identical to before
        assert plain == fixtures.golden_text(name, gold[0]["stdout"])
    st = harness.Setup(name, args + [tok], "chr1")
    perms, seed = (1000, 0) if tok == "--snn" else (int(tok[6:].split(",")[0]), int((tok[6:].split(",") + ["0"])[1]))
    assert (st.opts.snn, st.opts.snn_perms, st.opts.snn_seed) == (1, perms, seed)
    ctx = _lib.Context(engine.make_params(st.opts, st.sm), 0)
    kb = st.kbatch
    ref = np.ascontiguousarray(kb["ref"], dtype=np.uint8)
    k = np.ascontiguousarray(kb["k"], dtype=np.uint8 if ctx.k_bytes == 1 else np.uint16)
    rq = np.ascontiguousarray(kb["rmsq"], dtype=np.uint32)
    keys = np.ascontiguousarray(kb["keys"], dtype=np.uint16)
    L = len(ref)
    cmd = engine._Cmd(st.opts, st.sm, st.chr, st.beg, st.end)
    assert cmd.c.output == PBG_NUCDIV_SNN | perms << 1 | seed << 17
    rows = torch.zeros(L * ctx.row_bytes, dtype=torch.uint8, device="cuda")
    with _lib.Stream(ctx, [cmd.c], 0, L) as s:
        s.push(_lib.PbgPileup(L, 0, ref.ctypes.data, k.ctypes.data, rq.ctypes.data, None, keys.ctypes.data))
        s.finish()
        text = s.text(0)
        s.rows_into(rows.data_ptr(), rows.numel())
    assert text == ours
    wins = workload.reference_windows(st.beg, st.end, st.opts.win_size)
    types, flags = harness.rows_to_sites(rows.cpu().numpy(), ctx.row_bytes, L, st.sm.n)
    groups = default_groups(len(st.masks))
    got = _run_snn(ctx, rows, L, wins, groups, perms, seed, 0)   # rows are contig positions here: key0 = 0
    res = ref_snn(types, flags, st.sm.n, st.masks, wins, groups, perms, seed, 0)
    _assert_same(got, res, name)
    seg = (np.asarray(flags) & SEG) > 0
    seg_rows = [int(seg[a:b].sum()) for a, b in wins]
    assert max(seg_rows) > 1
    want = _want_text(plain, st.sm.pops, perms, seg_rows, res[1], res[3])
    assert ours == want
    assert ("psnn[" in ours) and ((("\t" + NA) in ours.split("psnn[")[1]) == (perms == 0 or not seg_rows[0]))
    # blocks of two windows: several streams, the same text
    monkeypatch.setenv("POPBAM_BLOCK_SITES", "2000")
    assert cli.run(base[0], base[1:] + [tok] + tail) == ours
    e = dict(os.environ, POPBAM_BLOCK_SITES="2000")
    e.pop("WORLD_SIZE", None)
    r = subprocess.run([os.path.join(REPO, "bin", "popbam"), *base, tok, *tail], capture_output=True, timeout=120, env=e)
    assert r.returncode == 0 and r.stdout.decode() == ours, r.stderr.decode()
    assert len(wins) > 2
    ctx.close()


@pytest.mark.gpu
def test_snn_appends_nothing_for_one_population(gpu_lib):
    d = fixtures.load_case("g14_onepop")["dir"]
    base = ["-f", os.path.join(d, "ref.fa"), "-w", "1"]
    tail = [os.path.join(d, "in.bam"), "chr1"]
    plain = cli.run("nucdiv", base + tail)
    assert plain and cli.run("nucdiv", base + ["--snn=50,1"] + tail) == plain
    rc, nat, err = _native(["nucdiv"] + base + ["--snn=50,1"] + tail)
    assert rc == 0 and nat == plain, err


@pytest.mark.gpu
@pytest.mark.parametrize("L,W", [(64 * 200, 1000), (64 * 20, 20)], ids=["w1000", "w20"])
def test_snn_on_a_synthetic_stream_ignores_min_sites(gpu_lib, L, W):
    """A streamed `nucdiv -w W --snn=64,9` over a synthetic batch pushed in several pieces, from a region
    that does not start at 0: the columns are the checker's with key0 = the contig position of row 0, and
    -k larger than any window blanks the reference's columns, not these.  With W = 20 most windows have no
    segregating site and print NA in both columns."""
    import torch
    from popbam_amd import _lib, workload
    n, masks, pos0 = 24, _blocks([8, 8, 8]), 64 * 50
    ctx = _lib.Context(_params(n, masks), 0)
    syn = workload.SynthPileup(ctx, L, 10, SEED + 5, pos0=pos0)
    hp = workload.HotPath(ctx, syn, [(0, L)], 0)
    hp.call()
    ctx.sync_check()
    host = hp.to_host()
    names = [f"p{i}" for i in range(3)]
    keep = [b"chr1", (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)]), (C.c_char_p * 3)(*[x.encode() for x in names])]

    def run(out_bits, min_sites):
        c = _lib.PbgCmd()
        c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq = 4, out_bits, min_sites, 10, 1   # PBG_CMD_NUCDIV
        c.windowed, c.win_size, c.beg, c.end = 1, W, pos0, pos0 + L
        c.chr_name = keep[0]
        c.sample_names = C.cast(keep[1], C.POINTER(C.c_char_p))
        c.pop_names = C.cast(keep[2], C.POINTER(C.c_char_p))
        c.refid = b"ref"
        rows = torch.zeros_like(hp.rows)
        with _lib.Stream(ctx, [c], pos0, L, 64 * 100) as st:
            st.push(_lib.PbgPileup(L, pos0, host["ref"].data_ptr(), host["k"].data_ptr(), host["rmsq"].data_ptr(),
                                   host["block_off"].data_ptr(), host["keys"].data_ptr()))
            st.finish()
            text = st.text(0)
            st.rows_into(rows.data_ptr(), rows.numel())
        return text, rows

    bits_ = _lib.PBG_NUCDIV_SNN | 64 << 1 | 9 << 17
    types, flags = harness.rows_to_sites(hp.rows.cpu().numpy(), ctx.row_bytes, L, n)
    wins = [(a - pos0, b - pos0) for a, b in workload.reference_windows(pos0, pos0 + L, W)]
    groups = default_groups(3)
    res = ref_snn(types, flags, n, masks, wins, groups, 64, 9, pos0)
    seg = (np.asarray(flags) & SEG) > 0
    seg_rows = [int(seg[a:b].sum()) for a, b in wins]
    for min_sites in (10, 10 * W):
        plain, rows0 = run(0, min_sites)
        ours, rows = run(bits_, min_sites)
        assert torch.equal(rows, rows0) and torch.equal(rows, hp.rows)
        assert ours == _want_text(plain, names, 64, seg_rows, res[1], res[3])
        assert (("pi[p0]:\t" + NA) in plain) == (min_sites > W) and "snn[*]:\t0." in ours
        assert (("snn[*]:\t" + NA) in ours) == (W == 20) == (min(seg_rows) == 0)
    ctx.close()
