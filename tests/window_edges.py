"""Helpers of the window-statistics edge tests (test_window_edges.py).

pack / founder_bits / flags_for / win_exact   crafted rows: sample bits -> the oracle's types, flags
                   (2 = counted, 6 = counted and segregating) and windows with an exact number of
                   segregating rows
census             which path window_stats_kernel, window_zns_kernel and window_ld_kernel take for a
                   window list, computed on the CPU from the limits restated below
case               the named inputs of test_window_edges.py with their oracle texts, built once per
                   process (the bounds-build child process rebuilds them by name)
run_case           a case through pbg_window_stats, one call per statistic, the pbg_format text of each
                   equal to the oracle's."""
import ctypes as C
import functools

import numpy as np

import harness
from window_helpers import oracle_text, window_text

# ---- the statistics kernels' limits, restated from the source
SEGCAP_MAX = 256            # pbg_common.h:274 kSegCap: segregating rows a window keeps in LDS, at most
SEGCAP_TIERS = ((2048, 64), (8192, 128))   # api.cpp:616: longest window <= 2048 rows: 64, <= 8192: 128, else kSegCap
WRAP = 65536                # stats_kernel.hip:154 `S < 65536u`, :256 / :386 / :513 / :529 `& 0xFFFF`: u16 differences
R2_LD_LDS = 4096            # stats_kernel.hip:642, :646 window_ld_kernel: r^2 doubles its LDS copy holds
R2_ZNS_LDS = 4608           # stats_kernel.hip:1023 launch_window_stats: r^2 doubles window_zns_kernel keeps in LDS
ZNS_GROUPS = 2              # stats_kernel.hip:794 PBG_ZNS_GROUPS
ZNS_MAX_C = 60 // ZNS_GROUPS   # stats_kernel.hip:797 kZnsMaxC: chains per workgroup
ZNS_R = 8                   # stats_kernel.hip:798 kZnsR: rounds per phase
ZNS_RING_STRIDE = 18        # stats_kernel.hip:799 kZnsRingStride: doubles per (round, chain)
ZNS_BUDGET = 75 * 1024      # stats_kernel.hip:1028: LDS bytes of a ZnS workgroup
ZNS_CHAIN_LIST = 256        # stats_kernel.hip:1030: list entries per chain the chain count is sized for
ZNS_CAP_MAX = 4096          # stats_kernel.hip:1035: LDS list entries per chain, at most
ZNS_COMPACT_N = 26          # stats_kernel.hip:1037: compacted lists up to this population size
ZNS_FIXED_MIN = 1 << 20     # api.cpp:634: fixed-place lists of up to this many words whatever the need
POOL_MAX = 512 << 20        # api.cpp:115 kPoolMax (words)

S_NUCDIV, S_SFS, S_ZNS, S_OMEGA, S_WALL, S_DIV_IND, S_DIV_POP = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
S_HAP_K, S_HAP_EHHS, S_HAP_DXY, S_TREE = 0x80, 0x100, 0x200, 0x400
F_OUTGROUP = 0x40
N_CU = 256                  # the CU count the CPU tests assume (the GPU tests read the device's)
# omega_max is O(S^3) in one lane of window_ld_kernel.  Measured on an MI355X, a tier case whose list holds the
# 513-row window took 5.6 s (12 samples) to 12.9 s (96 samples) against 1.3 to 2.0 s without it, so omega_max runs on
# windows of up to 300 rows; the windows of segcap - 1, segcap and segcap + 1 rows of every tier are among them
OMEGA_MAX_S = 300

from test_gpu_scale import STATS   # noqa: E402  (PBG_S_* flag, popbam_func_t, -o, min_freq, jc)

NO_OMEGA = [s for s in STATS if s[0] != S_OMEGA]


def segcap_for(maxlen):
    """Segregating rows per window in LDS for a list whose longest window has maxlen rows (api.cpp:616)."""
    for lim, cap in SEGCAP_TIERS:
        if maxlen <= lim:
            return cap
    return SEGCAP_MAX


def row_bytes_for(n):
    """include/popbam_gpu.h: 2-, 4-, 8- and 16-byte rows (two flag bits beside the sample bits)."""
    return 2 if n <= 14 else 4 if n <= 30 else 8 if n <= 62 else 16


# ---- crafted rows
def pack(bits):
    """Sample bits [L, n] -> types as harness.oracle_call returns them ([L] u64, [L, 2] above 64 samples)."""
    L, n = bits.shape
    b = np.zeros((L, 128), np.uint8)
    b[:, :n] = bits
    w = np.packbits(b, axis=1, bitorder="little").view(np.uint64).reshape(L, 2)
    return np.ascontiguousarray(w) if n > 64 else w[:, 0].copy()


def unpack(types, n):
    t = np.asarray(types, np.uint64)
    if t.ndim == 1:
        t = np.stack([t, np.zeros(len(t), np.uint64)], axis=1)
    return np.unpackbits(np.ascontiguousarray(t).view(np.uint8).reshape(len(t), 16), axis=1, bitorder="little")[:, :n]


def founder_bits(rng, L, n, founders, stretch, p=0.4):
    """Every sample copies one of `founders` haplotypes (each site derived with probability p in a
    founder); the copy source is redrawn every `stretch` rows."""
    out = np.zeros((L, n), np.uint8)
    for r0 in range(0, L, stretch):
        rows = min(stretch, L - r0)
        src = rng.integers(0, founders, n)
        out[r0:r0 + rows] = (rng.random((rows, founders)) < p).astype(np.uint8)[:, src]
    return out


def flags_for(rng, bits, p_nonseg=0.05, p_uncounted=0.03):
    """Flags of crafted bits.  Every third row (r % 3 == 2) is counted only, as are rows without a
    derived sample and p_nonseg of the others (their bits cleared); p_uncounted of the other rows are
    not counted at all.  A window of 10 or more counted rows then has fewer than 3/4 of them
    segregating, which keeps every Jukes-Cantor distance of `tree -d jc` defined (tree_jc_defined).
    Changes `bits`."""
    L = len(bits)
    third = np.arange(L) % 3 == 2
    seg = bits.any(axis=1) & (rng.random(L) >= p_nonseg) & ~third
    counted = seg | third | (rng.random(L) >= p_uncounted)
    bits[~seg] = 0
    return np.where(seg, 6, np.where(counted, 2, 0)).astype(np.uint8)


def win_exact(flags, start, S):
    """The shortest window from `start` with exactly S segregating rows (S = 0: the counted-only run
    at `start`, which must be there)."""
    seg = (flags[start:] & 4) > 0
    if S == 0:
        k = int(np.argmax(seg)) if seg.any() else len(seg)
        assert k > 0
        return (start, start + k)
    at = np.flatnonzero(seg)
    assert len(at) >= S, (start, S, len(at))
    return (start, start + int(at[S - 1]) + 1)


def make_params(n, sizes=None, interleave=0, flag=0):
    """Contiguous populations of the given sizes (default: two halves), or `interleave` populations
    dealt round-robin over the samples."""
    from popbam_amd import workload
    if interleave:
        masks = [0] * interleave
        for v in range(n):
            masks[v % interleave] |= 1 << v
    else:
        sizes = sizes or [n // 2, n - n // 2]
        assert sum(sizes) == n
        masks, at = [], 0
        for s in sizes:
            masks.append(((1 << s) - 1) << at)
            at += s
    p = workload.default_params(n, len(masks), flag=flag)
    for i, m in enumerate(masks):
        p.set_pop_mask(i, m)
        p.pop_n[i] = bin(m).count("1")
    return p


def pops_of(params):
    """([members of population i, ascending], ...)."""
    n = params.n_samples
    return [[v for v in range(n) if (params.get_pop_mask(i) >> v) & 1] for i in range(params.n_pops)]


# ---- census
def zns_plan(pop_n, n_win, n_cu):
    """launch_window_stats' arithmetic for window_zns_kernel (stats_kernel.hip:1018-1039): the r^2 doubles
    in LDS, C chains per workgroup, `cap` list entries per chain in LDS, and whether lists are compacted."""
    r2_total = sum((x + 1) ** 3 for x in pop_n)
    r2_lds = r2_total if r2_total <= R2_ZNS_LDS else 0
    chains = n_win * len(pop_n)
    tab = (((r2_lds + 2) & ~1) if r2_lds else 0) * 8
    per_chain = 2 * ZNS_R * ZNS_RING_STRIDE * 8 + ZNS_CHAIN_LIST * 4
    cfit = (ZNS_BUDGET - tab) // per_chain if ZNS_BUDGET > tab + per_chain else 1
    C_ = max(1, min(ZNS_MAX_C, cfit, (chains + 2 * n_cu - 1) // max(1, 2 * n_cu)))
    fixed = tab + 2 * ZNS_R * C_ * ZNS_RING_STRIDE * 8
    cap = (min(ZNS_CAP_MAX, (ZNS_BUDGET - fixed) // (C_ * 4)) & ~7) if ZNS_BUDGET > fixed else 0
    compact = bool(max(pop_n) <= ZNS_COMPACT_N and r2_lds and cap >= 16)
    return {"r2_total": r2_total, "r2_lds": r2_lds, "C": C_, "cap": cap if compact else 0, "compact": compact}


def census(types, flags, params, wins, stats, n_cu=N_CU):
    """The path decisions of one pbg_window_stats call with statistics mask `stats`, per window unless
    said otherwise.

    segcap (scalar), S, num_sites, over (S > segcap), nwords
    fast_sums          calc_nucdiv's sums from per-site counts (stats_kernel.hip:154-162)
    plane_n            samples whose bitplanes are built (:164-166); gather: the per-lane gather (:223);
                       planes_lds: bitplanes in LDS, not in the window's pool slice (:219)
    V1, V2             [n_win, n_pops] variable sites of each chain at min_freq 1 and 2
    r2_total (scalar), r2_ld_lds / r2_zns_lds: the r^2 tables in window_ld_kernel's / window_zns_kernel's LDS
    zns                zns_plan(); zns_fixed: lists at fixed places (api.cpp:630-637);
    wg_fits1, wg_fits2 per ZnS workgroup (C consecutive chains): every list within cap (s_fits, :853)
    pool_worst         the pool words the plan reserves (api.cpp:617-622)"""
    n, npop = params.n_samples, params.n_pops
    pop_n = [int(params.pop_n[i]) for i in range(npop)]
    members = pops_of(params)
    mw = 2 if row_bytes_for(n) == 16 else 1
    wins = np.asarray(wins, np.int64).reshape(-1, 2)
    lens = np.maximum(wins[:, 1] - wins[:, 0], 0)
    nw = len(wins)
    segcap = segcap_for(int(lens.max()))
    seg = (np.asarray(flags) & 4) > 0
    cnt = (np.asarray(flags) & 2) > 0
    assert not (seg & ~cnt).any(), "segregating rows are counted rows"

    def per_window(a):
        cs = np.concatenate([[0], np.cumsum(a, axis=0)]) if a.ndim == 1 else np.concatenate(
            [np.zeros((1,) + a.shape[1:], np.int64), np.cumsum(a, axis=0)])
        return np.where((lens > 0).reshape((-1,) + (1,) * (a.ndim - 1)), cs[wins[:, 1]] - cs[wins[:, 0]], 0)
    S = per_window(seg.astype(np.int64))
    num_sites = per_window(cnt.astype(np.int64))
    nwords = np.where(S > 0, (S + 63) // 64, 1)
    over = S > segcap
    # fast_sums
    last, ordered = -1, True
    for m in members:
        if m:
            ordered &= m[0] > last
            last = m[-1]
    sums = bool(stats & (S_NUCDIV | S_HAP_DXY))
    cost_pairs = sum((pop_n[a] * pop_n[b] + 63) // 64 for a in range(npop) for b in range(a, npop))
    fast = np.zeros(nw, bool)
    if sums and not (stats & S_HAP_DXY) and ordered:
        fast = (S < WRAP) & (npop * (npop + 1) // 2 * ((S + 63) // 64) <= cost_pairs * nwords)
    zbits = bool(stats & (S_HAP_K | S_HAP_EHHS))
    all_n = bool(stats & (S_DIV_IND | S_HAP_DXY | S_TREE))
    plane_n = np.where(all_n | (bool(stats & S_NUCDIV) & ~fast), n, min(n, max(pop_n)) if zbits else 0)
    gather = (plane_n > 0) & (nwords == 1) & (S * ((plane_n + 63) // 64) < plane_n)
    planecap = n * (segcap // 64)
    planes_lds = (plane_n > 0) & (n * nwords <= planecap)
    # variable sites per chain
    bits = unpack(types, n).astype(np.int64)
    m = np.stack([bits[:, mem].sum(axis=1) for mem in members], axis=1)   # [L, npop]
    pn = np.array(pop_n)
    V = [per_window((seg[:, None] & (m >= mf) & (m <= pn - mf)).astype(np.int64)) for mf in (1, 2)]
    zp = zns_plan(pop_n, nw, n_cu)
    need = int(mw * npop * lens.sum())
    zs = mw * npop * max(int(lens.max()), 1)
    zns_fixed = nw * zs <= max(2 * need, ZNS_FIXED_MIN) and nw * zs <= POOL_MAX
    fits = []
    for v in V:
        ch = v.reshape(-1)
        fits.append(np.array([bool(zp["compact"]) and (ch[g:g + zp["C"]] <= zp["cap"]).all()
                              for g in range(0, len(ch), zp["C"])]))
    ld_ws = bool(stats & (S_OMEGA | S_WALL))
    worst = 0
    for ln in lens.tolist():
        if ld_ws or ln > segcap:
            worst += mw * ln + n * (ln // 64 + 1) + (mw * npop * ln if ld_ws else 0)
        if stats & S_ZNS:
            worst += mw * npop * ln
    return {"segcap": segcap, "S": S, "num_sites": num_sites, "over": over, "nwords": nwords, "fast_sums": fast,
            "plane_n": plane_n, "gather": gather, "planes_lds": planes_lds, "V1": V[0], "V2": V[1],
            "r2_total": zp["r2_total"], "r2_ld_lds": zp["r2_total"] <= R2_LD_LDS, "r2_zns_lds": zp["r2_lds"] != 0,
            "zns": zp, "zns_fixed": zns_fixed, "wg_fits1": fits[0], "wg_fits2": fits[1], "pool_worst": worst}


# ---- the named inputs of test_window_edges.py
def _seed(name):
    return [0xC0FFEE31] + [ord(c) for c in name]


def _interleave(a, b):
    out = []
    for i in range(max(len(a), len(b))):
        out += a[i:i + 1] + b[i:i + 1]
    return out


def _tier(n, longest, rng, interleave):
    """A list whose longest window has `longest` rows: a dense zone of founder rows with windows of
    exactly segcap - 1, segcap, segcap + 1, 2 segcap + 1 and 63, 64, 65 segregating rows, dealt out
    between short windows, and a sparse zone that holds the longest window."""
    segcap = segcap_for(longest)
    D = 1800
    L = D + longest + 40
    bits = founder_bits(rng, L, n, 5, 48)
    flags = flags_for(rng, bits)
    thin = np.arange(L) >= D
    drop = thin & (rng.random(L) >= (1 / 64 if longest < 8000 else 1 / 200)) & (flags == 6)
    drop[:12] = True
    bits[drop] = 0
    flags[drop & (flags == 6)] = 2
    dense = [win_exact(flags, int(rng.integers(12, 300)), s)
             for s in (segcap - 1, segcap, segcap + 1, 2 * segcap + 1, 63, 64, 65)]
    sparse = [(a, a + int(rng.integers(6, 40))) for a in rng.integers(12, D - 50, 5).tolist()]
    sparse += [(D + 20, D + 20 + longest), (5, 5), (0, 12), (D + 100, D + 600)]
    assert max(b - a for a, b in dense) < longest
    return make_params(n, interleave=2 if interleave else 0), bits, flags, _interleave(dense, sparse), STATS, {}


def _gather(n, rng):
    """Windows of exactly S segregating rows around the per-lane gather's limit S ceil(plane_n / 64) <
    plane_n, for plane_n = n (diverge -o 0, haplo -o 2, tree) and the largest population (haplo -o 0/1)."""
    params = make_params(n)
    L = 600
    bits = founder_bits(rng, L, n, 5, 40)
    flags = flags_for(rng, bits)
    bits[:12] = 0
    flags[:12] = 2
    want = {0, 1, 2}
    for pl in (n, max(params.pop_n[i] for i in range(params.n_pops))):
        lim = (pl + (pl + 63) // 64 - 1) // ((pl + 63) // 64)   # the smallest S that leaves the gather
        want |= {lim - 1, lim}
    if n >= 70:
        want |= {62, 63}
    # (windows of up to 12 rows start at the 12 counted-only rows: at least min_sites counted rows in each)
    wins = [win_exact(flags, 0 if s <= 12 else int(rng.integers(0, 60)), s) for s in sorted(want)]
    return params, bits, flags, wins, STATS, {"min_snps": 0}


def _wrap(n, rng, interleave):
    """u16 wrap: in an X row sample a alone of population 0 and every sample of population 1 are derived.
    A window of c X rows has S = c, c differences between a and its population's other samples, c
    derived rows of a and Fixed[p1] = c: windows of 65535, 65536 and 65537 X rows, counted-only rows
    between them.  Three more windows run on into founder rows in which sample b copies a: S is beyond
    65536 there while a and b still differ at exactly 65535 / 65536 / 65537 rows."""
    params = make_params(n, interleave=2 if interleave else 0)
    p0, p1 = pops_of(params)
    a, b = p0[0], p0[1]
    NX, NF = WRAP + 1, 1500
    xz = np.zeros((NX + 500, n), np.uint8)
    fl = np.full(NX + 500, 2, np.uint8)
    at = np.sort(rng.choice(NX + 500, NX, replace=False))
    xz[np.ix_(at, [a] + p1)] = 1
    fl[at] = 6
    fb = founder_bits(rng, NF, n, 4, 50)
    fb[:, b] = fb[:, a]
    ff = flags_for(rng, fb)
    bits, flags = np.concatenate([xz, fb]), np.concatenate([fl, ff])
    L = len(bits)
    wins = [win_exact(flags, 0, c) for c in (WRAP - 1, WRAP, WRAP + 1)]
    T0 = len(xz)
    wins += [(int(at[k]), L) for k in (2, 1, 0)]
    wins += [(T0, L), (T0 + 100, T0 + 700), (T0 + 650, T0 + 1400), (T0 + 300, T0 + 390)]   # founder rows alone
    # ZnS at min_freq 1 and omega_max are left out: every X row is variable in population 0, and a chain
    # of 65,536 sites is 2 x 10^9 dependent additions on the device and as many table reads on the oracle
    # `tree -d jc` is left out as well: a and b differ at nearly every counted row (tree_jc_defined)
    stats = [s for s in NO_OMEGA if not (s[0] == S_ZNS and s[3] == 1) and not (s[0] == S_TREE and s[4] == 1)]
    return params, bits, flags, wins, stats, {"pair": (a, b), "x_rows": at}


def _nhaps(n, sizes, interleave, rng):
    """Few founders, so classes of three and more samples; windows inside and across the stretches."""
    params = make_params(n, sizes, interleave)
    L, stretch = 2400, 40
    bits = founder_bits(rng, L, n, 3 if n <= 24 else 4, stretch)
    flags = flags_for(rng, bits)
    wins = [(k * stretch + 4, k * stretch + 30) for k in range(0, 24, 2)]
    wins += [(k * stretch + 20, k * stretch + 20 + ln) for k, ln in ((1, 60), (5, 100), (9, 90), (13, 45), (17, 200))]
    wins += [(1000, 1999), (30, 30)]
    return params, bits, flags, wins, STATS, {}


def _subset(rng, mem, f):
    return sorted(rng.choice(mem, f, replace=False).tolist())


def _ehhs(n, sizes, rng):
    """Per window and population: two non-singleton columns (f derived members each, 1 < f < n_i - 1)
    repeated equally often, so only the value order decides which is the most repeated partition;
    above 64 samples some pairs are equal in the low word.  A singleton column, one with n_i - 1 derived
    members, the full and the empty column are repeated more often and must be ignored."""
    params = make_params(n, sizes)
    pops = pops_of(params)
    blocks, wins = [], []
    at = 0
    for w in range(14):
        Lw = int(rng.integers(60, 100))
        blk = founder_bits(rng, Lw, n, 4, 16)
        for mem in pops:
            nn = len(mem)
            cols = []
            if nn >= 4:
                r = int(rng.integers(3, 7))
                fa = int(rng.integers(2, nn - 1))
                fb_ = int(rng.integers(2, nn - 1))
                ca = _subset(rng, mem, fa)
                if n > 64 and mem[-1] >= 64 and mem[0] < 64 and w % 2 == 0:
                    # equal in the low word: the same low members, other high members
                    low = [v for v in ca if v < 64]
                    hi = [v for v in mem if v >= 64]
                    ca = low + _subset(rng, hi, 2)
                    cb = low + _subset(rng, hi, 3)
                else:
                    cb = _subset(rng, mem, fb_)
                if ca == cb:
                    cb = mem[:2] if ca != mem[:2] else mem[1:3]
                cols += [(ca, r), (cb, r)]
                if w % 3 == 0:
                    cols.append((_subset(rng, mem, 2), r - 1))
            r2 = 8
            cols += [(mem[:1], r2), (mem[1:], r2), (mem, 2), ([], 2)]
            rows_ = [c for c, k in cols for _ in range(k)]
            free = np.flatnonzero((at + np.arange(Lw)) % 3 != 2)   # (flags_for keeps every third row of the whole array)
            place = rng.choice(free, len(rows_), replace=False)
            for p_, c in zip(place, rows_):
                blk[p_, mem] = 0
                blk[p_, c] = 1
        blocks.append(blk)
        wins.append((at, at + Lw))
        at += Lw
    bits = np.concatenate(blocks)
    flags = flags_for(rng, bits, 0.0, 0.03)
    wins += [(10, at - 10), (at // 2, at // 2)]
    return params, bits, flags, wins, STATS, {}


def _wall(n, sizes, rng):
    """Runs of identical and complementary columns, partitions that come back after others, and columns
    full or empty in one population but variable in the next (last_type is shared, Appendix A.9)."""
    params = make_params(n, sizes)
    pops = pops_of(params)
    L = 1500
    bits = np.zeros((L, n), np.uint8)
    seen = []

    def fresh():
        """A new column: variable in one population and full or empty in the others (their type does not
        reach last_type), or variable in all."""
        c = (rng.random(n) < rng.choice([0.2, 0.5, 0.8])).astype(np.uint8)
        if rng.random() < 0.7:
            keep = int(rng.integers(0, len(pops)))
            for i, mem in enumerate(pops):
                if i != keep:
                    c[mem] = int(rng.integers(0, 2))
        return c
    cur = fresh()
    for r in range(L):
        u = rng.random()
        if u < 0.30:
            pass
        elif u < 0.50:
            cur = 1 - cur
        elif u < 0.65 and seen:
            cur = seen[int(rng.integers(0, len(seen)))].copy()
        else:
            cur = fresh()
        seen.append(cur.copy())
        bits[r] = cur
    flags = flags_for(rng, bits, 0.0, 0.03)
    bits[:12] = 0
    flags[:12] = 2
    wins = [win_exact(flags, 0, s) for s in (0, 1, 2)]
    wins += [(a, a + ln) for a, ln in zip(range(20, L - 200, 97), [30, 60, 120, 200, 45, 80, 150] * 3)]
    return params, bits, flags, wins, STATS, {}


def _zns_rows(rng, L, n):
    """Founder rows in which 2..n-2 samples are derived: variable at min_freq 1 and 2 alike."""
    out = np.zeros((0, n), np.uint8)
    while len(out) < L:
        b = founder_bits(rng, 2 * L, n, 6, 64)
        m = b.sum(axis=1)
        out = np.concatenate([out, b[(m >= 2) & (m <= n - 2)]])
    return out[:L]


def _zns_two(V, rng):
    """Two windows of V variable rows each, one population of 12: C = 1, cap = 4096."""
    n = 12
    bits = _zns_rows(rng, ZNS_CAP_MAX + 1 + 5, n)
    flags = np.full(len(bits), 6, np.uint8)
    return make_params(n, [n]), bits, flags, [(0, V), (5, 5 + V)], NO_OMEGA, {}


def _zns_many(equal, n_cu, rng):
    """More than 4 n_cu chains, all tiny but one of 4097 variable rows; `equal`: every window has the
    long one's length (lists at fixed places), else short ragged windows (pooled lists)."""
    n = 12
    nw = 4 * n_cu + 76
    V = ZNS_CAP_MAX + 1
    step = 8
    tail = founder_bits(rng, nw * step + V + 64, n, 6, 64)
    tf = flags_for(rng, tail, 0.0, 0.03)
    thin = (rng.random(len(tail)) >= (1 / 400 if equal else 1 / 100)) & (tf == 6)
    tail[thin] = 0
    tf[thin] = 2
    bits = np.concatenate([_zns_rows(rng, V, n), tail])
    flags = np.concatenate([np.full(V, 6, np.uint8), tf])
    if equal:
        wins = [(V + k * step, 2 * V + k * step) for k in range(nw - 1)]
    else:
        wins = [(V + k * step, V + k * step + int(ln)) for k, ln in enumerate(rng.integers(700, 2000, nw - 1))]
    wins.insert(nw // 3, (0, V))
    return make_params(n, [n]), bits, flags, wins, NO_OMEGA, {"min_snps": 0}


def _r2(sizes, rng):
    n = sum(sizes)
    bits = founder_bits(rng, 1500, n, 6, 32)
    flags = flags_for(rng, bits)
    wins = [(a, a + ln) for a, ln in zip(range(10, 1300, 110), [60, 90, 150, 75, 120, 40] * 2)]
    return make_params(n, sizes), bits, flags, wins, STATS, {}


SHORT_V = (0, 1, 2, 3, 16, 17, 33)


def _short(n, rng):
    """Windows with exactly (V0, V1) rows variable in population 0 / 1, every V of SHORT_V in each
    population, against 0 (monomorphic), the same and another V in the other."""
    params = make_params(n)
    p0, p1 = pops_of(params)
    pairs = [(v, 0) for v in SHORT_V] + [(0, v) for v in SHORT_V[1:]] + [(v, v) for v in SHORT_V[1:]]
    pairs += [(16, 17), (17, 33), (33, 3), (2, 16)]
    blocks, fl, wins, at = [], [], [], 0

    def var(mem):
        f = int(rng.integers(1, len(mem)))
        c = np.zeros(len(mem), np.uint8)
        c[rng.choice(len(mem), f, replace=False)] = 1
        return c
    for v0, v1 in pairs:
        both = min(v0, v1)
        kinds = ["b"] * both + ["0"] * (v0 - both) + ["1"] * (v1 - both) + ["n"] * 4 + ["c"] * 12
        kinds = [kinds[i] for i in rng.permutation(len(kinds))]
        blk = np.zeros((len(kinds), n), np.uint8)
        f = np.full(len(kinds), 6, np.uint8)
        for r, k in enumerate(kinds):
            if k == "c":
                f[r] = 2
                continue
            x = int(rng.integers(0, 2))
            blk[r, p0] = var(p0) if k in "b0" else x
            blk[r, p1] = var(p1) if k in "b1" else 1 - x if k == "n" else int(rng.integers(0, 2))
        blocks.append(blk)
        fl.append(f)
        wins.append((at, at + len(kinds)))
        at += len(kinds)
    return params, np.concatenate(blocks), np.concatenate(fl), wins, STATS, {"pairs": pairs, "min_snps": 0}


def _outgroup(n, outidx, rng):
    params = make_params(n, flag=F_OUTGROUP)
    bits = founder_bits(rng, 1600, n, 5, 40)
    flags = flags_for(rng, bits)
    wins = [(a, a + 100) for a in range(0, 1500, 100)] + [(0, 1600), (7, 7)]
    stats = [s for s in STATS if s[0] in (S_SFS, S_DIV_POP)]
    return params, bits, flags, wins, stats, {"outidx": outidx}


class Case:
    """Named rows, windows and statistics, with the oracle's text per statistic."""

    def __init__(self, name, params, bits, flags, wins, stats, extra):
        self.name, self.params, self.flags = name, params, np.ascontiguousarray(flags, np.uint8)
        self.n = params.n_samples
        assert not bits[(self.flags & 4) == 0].any()
        self.types = pack(bits)
        self.wins = [(int(a), int(b)) for a, b in wins]
        self.stats = list(stats)
        self.extra = extra
        self.outidx = extra.get("outidx", 0)
        self.min_snps = extra.get("min_snps", 10)
        self._text = {}

    def wins_for(self, st):
        """The case's windows; for omega_max those of at most OMEGA_MAX_S segregating rows (their longest
        window gives the same segcap)."""
        if st[0] != S_OMEGA:
            return self.wins
        seg = np.concatenate([[0], np.cumsum((self.flags & 4) > 0)])
        keep = [w for w in self.wins if w[1] <= w[0] or seg[w[1]] - seg[w[0]] <= OMEGA_MAX_S]
        assert segcap_for(max(b - a for a, b in keep)) == segcap_for(max(b - a for a, b in self.wins))
        return keep

    def oracle(self, st):
        if st not in self._text:
            stat, cmd_id, output, min_freq, jc = st
            self._text[st] = oracle_text(self.params, self.types, self.flags, cmd_id, output, self.wins_for(st),
                                         min_freq, jc, self.min_snps, self.outidx)
        return self._text[st]

    def census(self, stats, n_cu=N_CU):
        return census(self.types, self.flags, self.params, self.wins, stats, n_cu)


@functools.lru_cache(maxsize=None)
def case(name, n_cu=N_CU):
    """family-arguments, e.g. 'T-2048-12', 'T-2049-12i', 'G-24', 'W-4', 'W-96i', 'H-63.2', 'H-i3-96', 'E-3.4',
    'L-6.6', 'Z-4096', 'Z-eq', 'Z-rag', 'R-15.7', 'S-12', 'O-96-90' (sizes joined by dots; a trailing i:
    interleaved populations)."""
    parts = name.split("-")
    fam = parts[0]
    rng = np.random.default_rng(_seed(name))

    def n_il(s):
        return int(s.rstrip("i")), s.endswith("i")

    def sizes(s):
        return [int(x) for x in s.split(".")]
    if fam == "T":
        n, il = n_il(parts[2])
        r = _tier(n, int(parts[1]), rng, il)
    elif fam == "G":
        r = _gather(int(parts[1]), rng)
    elif fam == "W":
        n, il = n_il(parts[1])
        r = _wrap(n, rng, il)
    elif fam == "H":
        if parts[1].startswith("i"):
            r = _nhaps(int(parts[2]), None, int(parts[1][1:]), rng)
        else:
            r = _nhaps(sum(sizes(parts[1])), sizes(parts[1]), 0, rng)
    elif fam == "E":
        r = _ehhs(sum(sizes(parts[1])), sizes(parts[1]), rng)
    elif fam == "L":
        r = _wall(sum(sizes(parts[1])), sizes(parts[1]), rng)
    elif fam == "Z":
        r = _zns_many(parts[1] == "eq", n_cu, rng) if parts[1] in ("eq", "rag") else _zns_two(int(parts[1]), rng)
    elif fam == "R":
        r = _r2(sizes(parts[1]), rng)
    elif fam == "S":
        r = _short(int(parts[1]), rng)
    elif fam == "O":
        r = _outgroup(int(parts[1]), int(parts[2]), rng)
    else:
        raise KeyError(name)
    return Case(name, *r)


# ---- the oracle's text, taken apart
def cells(text):
    """[(line, label, value)] of a statistics text: the fields that follow a `label:` field."""
    out = []
    for li, line in enumerate(text.splitlines()):
        f = line.split("\t")
        out += [(li, a[:-1], b) for a, b in zip(f, f[1:]) if a.endswith(":")]
    return out


def dull_share(c, windows=None, skip=()):
    """Share of a case's printed statistic cells that are nan / NA / inf / 0.00000, over its statistics
    (and the given windows; labels that start with one of `skip` are not counted)."""
    tot = dull = 0
    for st in c.stats:
        if st[1] == 3:
            continue   # tree prints a tree, not labelled cells
        wl = c.wins_for(st)
        for li, lb, v in cells(c.oracle(st)):
            if (windows is not None and wl[li] not in windows) or (skip and lb.startswith(tuple(skip))):
                continue
            tot += 1
            dull += v.strip() in ("NA", "nan", "-nan", "0.00000", "inf", "-inf")
    return dull / max(tot, 1)


def tree_jc_defined(c):
    """Every Jukes-Cantor distance `tree -d jc` takes a logarithm of is below 3/4 (windows the command
    prints: at least 10 counted rows, a segregating one).  Beyond, -0.75 log(1 - 4p/3) is NaN, no pair
    of the neighbour joining compares below the minimum, and the reference's join_tree hooks up a
    cluster it has already emptied: undefined there, and in both restatements."""
    bits = unpack(c.types, c.n).astype(np.int32)
    seg = (c.flags & 4) > 0
    cnt = (c.flags & 2) > 0
    for a, b in c.wins:
        B = bits[a:b][seg[a:b]]
        ns = int(cnt[a:b].sum())
        if a >= b or ns < 10 or len(B) < 1:
            continue
        der = B.sum(axis=0)
        D = der[:, None] + der[None, :] - 2 * (B.T @ B)
        if 4 * (max(int(D.max()), int(der.max())) & 0xFFFF) >= 3 * ns:
            return False
    return True


# ---- the device
class _Out:
    def __init__(self, out):
        self.out = out


def run_case(name, stats=None):
    """The case through pbg_window_stats, one call per statistic on one context: the pbg_format text
    equals the oracle's, and pbg_check is clean after every call (a pool that ran out would be
    reported there).  Returns the number of calls."""
    import torch
    from popbam_amd import _lib, workload
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c = case(name, n_cu)
    ctx = _lib.Context(c.params, 0)
    try:
        L = len(c.flags)
        rows = torch.from_numpy(harness.rows_from_oracle(c.types, c.flags, ctx.row_bytes).copy()).cuda()
        for st in stats or c.stats:
            stat, cmd_id, output, min_freq, jc = st
            wins = c.wins_for(st)
            nw = len(wins)
            wt = torch.tensor([x for ab in wins for x in ab], dtype=torch.int32).reshape(-1, 2).cuda()
            out = workload.WindowOutputs(nw, c.n, c.params.n_pops, sfs_stride=ctx.sfs_stride)
            so = _lib.PbgStatOpts(stat, min_freq, c.outidx, jc)
            ost = out.struct(workload.HotPath.fields_for(stat))
            ctx.check(ctx.lib.pbg_window_stats(ctx.h, rows.data_ptr(), L, wt.data_ptr(), nw, C.byref(so), C.byref(ost),
                                               workload.stream_handle()), "pbg_window_stats")
            ctx.sync_check()
            gpu = window_text(ctx, c.params, _Out(out), cmd_id, output, wins, min_freq, jc, c.min_snps,
                              outidx=c.outidx)
            want = c.oracle(st)
            if gpu != want:
                bad = [(i, a, b) for i, (a, b) in enumerate(zip(gpu.splitlines(), want.splitlines())) if a != b]
                raise AssertionError(f"{name} statistic {st}: {len(bad)} lines differ, first window {bad[0][0]} "
                                     f"{wins[bad[0][0]]}:\n gpu    {bad[0][1][:600]}\n oracle {bad[0][2][:600]}")
        return len(stats or c.stats)
    finally:
        ctx.close()
