"""Window-statistics parity at the capacity edges and on haplotype structure.

The other window tests run window_stats_kernel, window_zns_kernel and window_ld_kernel on called
synthetic rows, whose sites are independent: the conditions at which stats_kernel.hip takes another
path are then met by accident of the data, and the branches written for haplotype structure see
trivial inputs (no two samples of a population alike, hardly a repeated column).  The inputs here
(window_edges.case) are crafted rows -- founder haplotypes, runs of identical and complementary
columns, exact counts -- with windows on both sides of every such condition:

  T   segcap tiers 64 / 128 / 256 (longest window 2048 / 2049 / 8192 / 8193 rows): windows of
      segcap - 1, segcap, segcap + 1 and 2 segcap + 1 segregating rows between short ones, so pool
      slices are handed out between LDS-only windows; 63 / 64 / 65 rows (one / two bitplane words)
  G   the per-lane bitplane gather against the ballots
  W   u16 wrap: a window, a sample pair, a Fixed count and a sample's derived count at 65535 / 65536 / 65537
  H   calc_nhaps' merge loop: classes of three and more samples, in registers and in LDS
  E   calc_ehhs' reduction: count ties only the value order breaks, also in the high word alone
  L   Wall's B and Q: repeated, complementary and returning partitions, the shared last_type
  Z   ZnS lists at the LDS list capacity; a long chain among short ones of its workgroup
  R   the r^2 tables in and out of LDS (4096 / 4608 doubles)
  S   ZnS / omega_max chains of 0, 1, 2, 3, 16, 17, 33 sites
  O   the outgroup flip of sfs and diverge -o 1

The CPU tests show with window_edges.census (the kernels' path decisions restated from the sources,
and checked against them) that each case reaches the path it is named for, on both sides of the
edge, and that the oracle's text is informative there; the GPU tests compare the whole pbg_format
text of every statistic with the oracle's (orc_windows_from_sites), on the product build and, for
T, W, H and Z, on the PBG_BOUNDS build."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import window_edges as we

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "popbam_amd", "csrc")
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")

TIERS = (2048, 2049, 8192, 8193)
T_CASES = [f"T-{ln}-{n}" for ln in TIERS for n in (12, 31, 63, 96, 126)]
P_CASES = ["T-2048-12i", "T-2049-14", "T-8192-15", "T-8193-96i"]   # plane statistics past segcap, interleaved too
G_CASES = ["G-12", "G-24", "G-70", "G-126"]
W_CASES = ["W-4", "W-12", "W-12i", "W-96", "W-96i"]
H_CASES = ["H-8.8.8", "H-63.2", "H-64.2", "H-65.2", "H-126", "H-2.65", "H-i2-12", "H-i3-96"]
E_CASES = ["E-6.6", "E-3.4", "E-48.48", "E-63.63"]
L_CASES = ["L-6.6", "L-8.8.8", "L-63.63"]
Z_TWO = ["Z-4095", "Z-4096", "Z-4097"]
Z_MANY = ["Z-eq", "Z-rag"]
R_CASES = ["R-15", "R-15.7", "R-15.8", "R-16", "R-12.12"]
S_CASES = ["S-12", "S-24"]
O_CASES = ["O-12-11", "O-12-0", "O-96-5", "O-96-90"]
BOUNDS_CASES = ["T-2049-12", "T-8193-96", "W-4", "W-96i", "H-65.2", "H-i3-96", "Z-4097", "Z-rag"]
ALL_CASES = T_CASES + P_CASES + G_CASES + W_CASES + H_CASES + E_CASES + L_CASES + Z_TWO + Z_MANY + R_CASES + S_CASES + O_CASES

PLANE_STATS = (we.S_NUCDIV, we.S_DIV_IND, we.S_HAP_K, we.S_HAP_EHHS, we.S_HAP_DXY, we.S_TREE)


def _values(c, st, label):
    """{window: value text} of the cells `label` in the oracle's text of statistic st."""
    return {li: v for li, lb, v in we.cells(c.oracle(st)) if lb == label}


def _stat(flag, min_freq=1, jc=0):
    return next(s for s in we.STATS if s[0] == flag and s[3] == min_freq and s[4] == jc)


# ---------------------------------------------------------------- CPU: the census is the sources'
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_census_constants_equal_the_sources():
    common, api, st = _src("pbg_common.h"), _src("api.cpp"), _src("stats_kernel.hip")

    def one(pattern, text):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return m[0]
    assert int(one(r"constexpr int kSegCap = (\d+);", common)) == we.SEGCAP_MAX
    tier = one(r"segcap = maxlen <= (\d+) \? (\d+) : maxlen <= (\d+) \? (\d+) : pbg::kSegCap;", api)
    assert tuple(int(x) for x in tier) == tuple(x for t in we.SEGCAP_TIERS for x in t)
    assert int(one(r"&& S < (\d+)u\)", st)) == we.WRAP
    assert len(re.findall(r"& 0xFFFFu?\b", st)) == 4   # pair_diff, Fixed, diverge -o 0, tree: u16 = WRAP - 1
    assert int(one(r"__shared__ double s_r2\[(\d+)\];", st)) == we.R2_LD_LDS
    assert int(one(r"const bool r2_lds = r2_total <= (\d+);", st)) == we.R2_LD_LDS
    assert int(one(r"const int r2_lds = r2_total <= (\d+) \? r2_total : 0;", st)) == we.R2_ZNS_LDS
    assert int(one(r"#define PBG_ZNS_GROUPS (\d+)", st)) == we.ZNS_GROUPS
    assert int(one(r"constexpr int kZnsMaxC = (\d+) / kZnsG;", st)) // we.ZNS_GROUPS == we.ZNS_MAX_C
    assert int(one(r"constexpr int kZnsR = (\d+);", st)) == we.ZNS_R
    assert int(one(r"constexpr int kZnsRingStride = (\d+);", st)) == we.ZNS_RING_STRIDE
    assert int(one(r"const size_t budget = (\d+) \* 1024;", st)) * 1024 == we.ZNS_BUDGET
    per = one(r"const size_t per_chain = \(size_t\)2 \* kZnsR \* kZnsRingStride \* 8 \+ (\d+) \* 4;", st)
    assert int(per) == we.ZNS_CHAIN_LIST
    assert int(one(r"std::min<size_t>\((\d+), \(budget - fixed\) / \(\(size_t\)C \* 4\)\) & ~7", st)) == we.ZNS_CAP_MAX
    assert int(one(r"const int compact = \(max_pop <= (\d+) && r2_lds && cap >= 16\)", st)) == we.ZNS_COMPACT_N
    assert one(r"std::max<uint64_t>\(2 \* need, (1 << \d+)\)", api) == "1 << 20" and we.ZNS_FIXED_MIN == 1 << 20
    assert int(one(r"constexpr uint64_t kPoolMax = (\d+)ull << 20;", api)) << 20 == we.POOL_MAX
    # the decisions the census restates, as the kernel writes them
    assert "fast_sums = np * (np + 1) / 2 * (int)((S + 63) / 64) <= cost_pairs * nwords;" in st
    assert "if (nwords == 1 && (int)S * ((plane_n + 63) / 64) < plane_n) {" in st
    assert "plane = (n * nwords <= L.planecap) ? s_plane : wpl;" in st
    assert "L.planecap = planes ? n * (segcap / 64) : 0;" in st
    assert "if (z.V > cap) atomicAnd(&s_fits, 0);" in st
    assert "(chains + 2 * n_cu - 1) / std::max(1, 2 * n_cu)" in st


def test_stats_are_test_gpu_scales():
    assert len(we.STATS) == 13 and len({s[0] for s in we.STATS}) == 11 and len(we.NO_OMEGA) == 12


# ---------------------------------------------------------------- CPU: every case takes its path
@pytest.mark.parametrize("name", T_CASES + P_CASES)
def test_tier_lists_put_windows_on_both_sides_of_segcap(name):
    c = we.case(name)
    longest = int(name.split("-")[1])
    cap = {2048: 64, 2049: 128, 8192: 128, 8193: 256}[longest]
    s = c.census(we.S_TREE)
    assert max(b - a for a, b in c.wins) == longest and s["segcap"] == cap
    S = s["S"].tolist()
    print(f"{name}: segcap {cap}, S per window {S}, pool words reserved {s['pool_worst']}")
    assert S[0:14:2] == [cap - 1, cap, cap + 1, 2 * cap + 1, 63, 64, 65]
    # omega_max runs on the windows of up to OMEGA_MAX_S rows: the same tier, a window past segcap among them
    om = c.wins_for(_stat(we.S_OMEGA))
    assert we.segcap_for(max(b - a for a, b in om)) == cap and len(om) >= len(c.wins) - 1
    assert any(x > cap for x, w in zip(S, c.wins) if w in om) and any(x == cap - 1 for x, w in zip(S, c.wins) if w in om)
    # pool slices between LDS-only windows: windows past segcap alternate with windows within it
    over = s["over"].tolist()
    assert over[0:8] == [False, False, False, False, True, False, True, False] and not any(over[1::2])
    assert (cap == 64) == over[12]   # 65 rows: past segcap only in the lowest tier
    # one and two bitplane words; the planes leave LDS exactly when the rows do
    assert s["nwords"].tolist()[8:14:2] == [1, 1, 2]
    for stat in PLANE_STATS:
        t = c.census(stat)
        need = t["plane_n"] > 0
        if stat != we.S_NUCDIV or name.endswith("i"):
            assert need.all()
        assert (t["planes_lds"][need] == ~t["over"][need]).all()
    # nucdiv: from per-site counts for contiguous populations, from sample pairs for interleaved ones
    fs = c.census(we.S_NUCDIV)["fast_sums"]
    assert not fs.any() if name.endswith("i") else fs.any()
    assert (s["num_sites"] > s["S"])[s["S"] > 20].all()   # counted rows that are not segregating


@pytest.mark.parametrize("name", G_CASES)
def test_gather_cases_sit_on_both_sides_of_the_gather(name):
    c = we.case(name)
    n = c.n
    for stat, pl in ((we.S_DIV_IND, n), (we.S_HAP_DXY, n), (we.S_TREE, n), (we.S_HAP_K, n // 2), (we.S_HAP_EHHS, n // 2)):
        s = c.census(stat)
        assert (s["plane_n"] == pl).all()
        lim = -(-pl // ((pl + 63) // 64))   # the smallest S with S ceil(plane_n / 64) >= plane_n
        by_s = dict(zip(s["S"].tolist(), s["gather"].tolist()))
        print(f"{name} statistic {stat:#x}: plane_n {pl}, gather up to S = {lim - 1}: {by_s}")
        assert by_s[lim - 1] is True and by_s[lim] is False
        assert by_s[0] and by_s[1] and by_s[2]
    if n >= 70:
        assert {62, 63} <= set(s["S"].tolist())


@pytest.mark.parametrize("name", W_CASES)
def test_wrap_cases_land_on_65536(name):
    c = we.case(name)
    a, b = c.extra["pair"]
    bits = we.unpack(c.types, c.n).astype(np.int64)
    seg = (c.flags & 4) > 0
    p0, p1 = we.pops_of(c.params)
    s = c.census(we.S_NUCDIV)
    S = s["S"].tolist()
    assert S[:3] == [we.WRAP - 1, we.WRAP, we.WRAP + 1] and all(x > we.WRAP for x in S[3:6])
    got = []
    for beg, end in c.wins[:6]:
        B = bits[beg:end][seg[beg:end]]
        got.append((int((B[:, a] != B[:, b]).sum()), int(B[:, a].sum()), int(B[:, p1].all(axis=1).sum())))
    print(f"{name}: S {S}, (differences of samples {a} and {b}, derived rows of {a}, rows fixed in p1) {got}")
    assert [g[0] for g in got] == [we.WRAP - 1, we.WRAP, we.WRAP + 1] * 2
    assert [g[1] for g in got[:3]] == [we.WRAP - 1, we.WRAP, we.WRAP + 1]
    assert [g[2] for g in got[:3]] == [we.WRAP - 1, we.WRAP, we.WRAP + 1]
    assert (s["num_sites"] > s["S"]).all()
    # the sums switch at S = 65536 for contiguous populations and never come from counts for interleaved ones
    assert s["fast_sums"].tolist()[:6] == ([False] * 6 if name.endswith("i") else [True] + [False] * 5)
    # what the wrap does to the text: at 65536 differences the two samples are one haplotype
    k = _values(c, _stat(we.S_HAP_K), "K[p0]")
    pi = _values(c, _stat(we.S_HAP_DXY), "pi[p0]")
    fx = _values(c, _stat(we.S_DIV_POP), "Fixed[p1]")
    assert [fx[w] for w in range(3)] == ["65535", "0", "1"]
    if c.n == 4:
        assert [k[w] for w in range(3)] == ["2", "1", "2"] and [pi[w] for w in range(3)] == ["65535.00000", "0.00000", "1.00000"]
    else:
        assert int(k[1]) < int(k[0]) == int(k[2])   # (with interleaved populations K counts other samples, A.11)
    assert not any(st[0] == we.S_OMEGA for st in c.stats)
    if not name.endswith("i") and c.n > 4:
        # Fay and Wu's H of population 0 (every X row a singleton there): calc_sfs multiplies
        # num_snps * (num_snps - 1) as int (pop_sfs.cpp:277), which wraps from 46,342 sites on
        h = _values(c, _stat(we.S_SFS), "H[p0]")
        nn = len(p0)
        a1, a2, a2n1 = sum(1.0 / j for j in range(1, nn)), sum(1.0 / (j * j) for j in range(1, nn)), \
            sum(1.0 / (j * j) for j in range(1, nn + 1))
        for w, S_ in enumerate(S[:3]):
            ss1 = (S_ * (S_ - 1)) & 0xFFFFFFFF
            ss1 -= (ss1 >> 31) << 32
            var = ((nn - 2) * (S_ / a1) / (6.0 * (nn - 1))) + ((ss1 / ((a1 * a1) + a2)) * (
                18.0 * (nn * nn) * (3.0 * nn + 2.0) * a2n1 - (88.0 * nn * nn * nn + 9.0 * (nn * nn) - 13.0 * nn + 6.0)) / (
                9.0 * nn * ((nn - 1) * (nn - 1))))
            fwh = S_ * ((1.0 / a1) - (1.0 / (nn - 1)))
            assert ss1 != S_ * (S_ - 1)
            assert h[w].strip() == ("NA" if var < 0 else "%.5f" % (fwh / var ** 0.5)), (w, h[w], var)


def _classes(c, pop, beg, end):
    """Sizes of the classes of identical samples of a population over a window's segregating rows."""
    bits = we.unpack(c.types, c.n)
    seg = (c.flags & 4) > 0
    sub = bits[beg:end][seg[beg:end]][:, pop]
    _, counts = np.unique(sub.T, axis=0, return_counts=True)
    return sorted(counts.tolist(), reverse=True)


@pytest.mark.parametrize("name", H_CASES)
def test_structure_cases_merge_samples(name):
    c = we.case(name)
    pops = we.pops_of(c.params)
    big = max(range(len(pops)), key=lambda i: len(pops[i]))
    nn = len(pops[big])
    wins = [w for w in c.wins if w[1] > w[0]]
    cls = [_classes(c, pops[big], a, b) for a, b in wins]
    three = sum(1 for x in cls if x[0] >= 3)
    both = sum(1 for x in cls if 2 <= len(x) < nn)
    print(f"{name}: population {big} of {nn}: windows with a class of 3+ samples {three}/{len(wins)}, "
          f"with 2 <= classes < n {both}/{len(wins)}")
    assert three >= 4 and both >= len(wins) // 2
    # the oracle's K (local indices into the global matrix, Appendix A.11: the first population's is the class count)
    k = _values(c, _stat(we.S_HAP_K), "K[p0]")
    n0 = len(pops[0])
    good = sum(1 for v in k.values() if v.strip() != "NA" and 2 <= int(v) < n0)
    if n0 > 2:
        assert good >= len(c.wins) // 2, (good, len(c.wins))
    # registers up to 64 samples, LDS beyond
    assert (nn > 64) == (name in ("H-65.2", "H-126", "H-2.65"))
    if len(pops) > 1:
        mins = [v for lb in {lb for _, lb, _ in we.cells(c.oracle(_stat(we.S_HAP_DXY)))} if lb.startswith("min[")
                for v in _values(c, _stat(we.S_HAP_DXY), lb).values()]
        assert "0" in mins
    # Wall's last_type is shared by the populations (Appendix A.9): a column repeats it only where
    # every other population is monomorphic, which populations of 8 and more founder copies never are
    if name in ("H-63.2", "H-64.2", "H-65.2", "H-2.65", "H-126"):
        walls = we.cells(c.oracle(_stat(we.S_WALL)))
        b = {(li, lb[2:]): v for li, lb, v in walls if lb.startswith("B[")}
        q = {(li, lb[2:]): v for li, lb, v in walls if lb.startswith("Q[")}
        num = [(float(b[x]), float(q[x])) for x in b if b[x].strip() not in ("NA", "nan", "-nan")]
        assert any(bb > 0 and qq > bb for bb, qq in num)
    e = [float(v) for _, lb, v in we.cells(c.oracle(_stat(we.S_HAP_EHHS))) if v.strip() not in ("NA", "nan", "-nan")]
    assert len(set(e)) > 3 and all(np.isfinite(e))


@pytest.mark.parametrize("name", E_CASES)
def test_ehhs_cases_tie_at_the_top(name):
    c = we.case(name)
    bits = we.unpack(c.types, c.n)
    seg = (c.flags & 4) > 0
    ties = hi_ties = ignored = 0
    for i, mem in enumerate(we.pops_of(c.params)):
        nn = len(mem)
        for beg, end in c.wins[:14]:
            sub = bits[beg:end][seg[beg:end]][:, mem]
            cols, cnt = np.unique(sub, axis=0, return_counts=True)
            f = cols.sum(axis=1)
            cand = (f > 1) & (f < nn - 1)
            if nn < 4:
                assert not cand.any()
                continue
            if not cand.any():
                continue
            top = cnt[cand].max()
            at_top = cols[cand][cnt[cand] == top]
            if len(at_top) >= 2 and len({int(x.sum()) for x in at_top}) >= 2:
                ties += 1
                lo = [j for j, v in enumerate(mem) if v < 64]
                if c.n > 64 and lo and len(lo) < nn and len({tuple(x[lo]) for x in at_top}) < len(at_top):
                    hi_ties += 1
            if cnt[~cand].max() > top:
                ignored += 1
    print(f"{name}: (window, population) with a count tie between columns of different frequency {ties}, "
          f"of those equal in the low word {hi_ties}, with a more repeated column to ignore {ignored}")
    e = [v.strip() for _, _, v in we.cells(c.oracle(_stat(we.S_HAP_EHHS)))]
    if name == "E-3.4":
        p0 = _values(c, _stat(we.S_HAP_EHHS), "EHHS[p0]")
        assert all(v.strip() == "NA" for v in p0.values())       # n_i < 4
        p1 = [v.strip() for v in _values(c, _stat(we.S_HAP_EHHS), "EHHS[p1]").values()]
        assert sum(v != "NA" for v in p1) >= 10
        assert ignored >= 8
        return
    assert ties >= 8 and ignored >= 8
    assert (hi_ties >= 3) == (c.n > 64)
    num = [float(v) for v in e if v != "NA"]
    assert len(num) >= 24 and all(np.isfinite(num)) and len(set(num)) >= 3


@pytest.mark.parametrize("name", L_CASES)
def test_wall_cases_repeat_and_return(name):
    c = we.case(name)
    s = c.census(we.S_WALL)
    assert s["S"].tolist()[:3] == [0, 1, 2]
    walls = we.cells(c.oracle(_stat(we.S_WALL)))
    b = {(li, lb[2:]): v for li, lb, v in walls if lb.startswith("B[")}
    q = {(li, lb[2:]): v for li, lb, v in walls if lb.startswith("Q[")}
    num = [(float(b[x]), float(q[x])) for x in b if b[x].strip() not in ("NA", "nan", "-nan")]
    print(f"{name}: (B, Q) of the first chains {num[:6]}")
    assert len(num) >= 20 and sum(bb > 0 and qq > bb for bb, qq in num) >= len(num) // 4
    assert len({x for x, _ in num}) > 6
    # rows full or empty in a population and variable in the next: last_type comes from another population
    bits = we.unpack(c.types, c.n)
    pops = we.pops_of(c.params)
    seg = (c.flags & 4) > 0
    m = [bits[:, p].sum(axis=1) for p in pops]
    mono0 = seg & ((m[0] == 0) | (m[0] == len(pops[0]))) & (m[1] > 0) & (m[1] < len(pops[1]))
    assert mono0.sum() >= 30


@pytest.mark.parametrize("name,V", [("Z-4095", 4095), ("Z-4096", 4096), ("Z-4097", 4097)])
def test_zns_two_windows_sit_at_the_list_capacity(name, V):
    c = we.case(name)
    for mf, key, fit in ((1, "V1", "wg_fits1"), (2, "V2", "wg_fits2")):
        s = c.census(we.S_ZNS)
        assert s["zns"]["C"] == 1 and s["zns"]["cap"] == we.ZNS_CAP_MAX and s["zns"]["compact"] and s["r2_zns_lds"]
        assert s[key].reshape(-1).tolist() == [V, V]
        assert s[fit].tolist() == [V <= we.ZNS_CAP_MAX] * 2
    print(f"{name}: C {s['zns']['C']}, cap {s['zns']['cap']}, V {V}, fixed-place lists {s['zns_fixed']}")


@pytest.mark.parametrize("name", Z_MANY)
def test_zns_long_chain_drags_its_workgroup(name):
    c = we.case(name)
    s = c.census(we.S_ZNS)
    z = s["zns"]
    nch = len(c.wins) * c.params.n_pops
    assert nch > 4 * we.N_CU and z["C"] >= 2 and z["cap"] == we.ZNS_CAP_MAX and z["compact"]
    assert s["zns_fixed"] == (name == "Z-eq")
    for key, fit in (("V1", "wg_fits1"), ("V2", "wg_fits2")):
        v = s[key].reshape(-1)
        long_ = np.flatnonzero(v > z["cap"])
        assert long_.tolist() == [len(c.wins) // 3] and v[long_[0]] == we.ZNS_CAP_MAX + 1
        g = long_[0] // z["C"]
        mates = v[g * z["C"]:(g + 1) * z["C"]]
        print(f"{name} {key}: C {z['C']}, the long chain's workgroup holds chains of {mates.tolist()} sites")
        assert len(mates) == z["C"] and (np.sort(mates)[:-1] <= 64).all()
        assert s[fit].tolist().count(False) == 1 and not s[fit][g]
        assert v.max() == we.ZNS_CAP_MAX + 1 and np.median(v) <= 16


@pytest.mark.parametrize("name,total,ld_lds,zns_lds", [("R-15", 4096, True, True), ("R-15.7", 4608, False, True),
                                                       ("R-15.8", 4825, False, False), ("R-16", 4913, False, False),
                                                       ("R-12.12", 4394, False, True)])
def test_r2_table_placement(name, total, ld_lds, zns_lds):
    s = we.case(name).census(we.S_ZNS)
    assert (s["r2_total"], s["r2_ld_lds"], s["r2_zns_lds"]) == (total, ld_lds, zns_lds)
    assert (s["S"] >= 20).all() and (s["S"] <= we.OMEGA_MAX_S).all()


@pytest.mark.parametrize("name", S_CASES)
def test_short_chains_have_the_asked_lengths(name):
    c = we.case(name)
    s = c.census(we.S_ZNS)
    assert [tuple(x) for x in s["V1"].tolist()] == c.extra["pairs"]
    for i in (0, 1):
        assert set(we.SHORT_V) <= set(s["V1"][:, i].tolist())
    mono_then_var = [(a, b) for a, b in c.extra["pairs"] if a == 0 and b > 0]
    assert len(mono_then_var) >= 6 and c.min_snps == 0


@pytest.mark.parametrize("name", O_CASES)
def test_outgroup_cases_flip_in_every_window(name):
    c = we.case(name)
    assert c.params.flag & we.F_OUTGROUP and [s[0] for s in c.stats] == [we.S_SFS, we.S_DIV_POP]
    out = we.unpack(c.types, c.n)[:, c.outidx].astype(bool) & ((c.flags & 4) > 0)
    per = [int(out[a:b].sum()) for a, b in c.wins if b > a]
    print(f"{name}: segregating rows at which the outgroup is derived, per window {per}")
    assert min(per) >= 10
    assert (c.outidx >= 64) == (name == "O-96-90")
    # the flip shows: the same rows without the flag print another text
    from window_helpers import oracle_text
    st = _stat(we.S_DIV_POP)
    plain = we.make_params(c.n)
    assert oracle_text(plain, c.types, c.flags, st[1], st[2], c.wins, 1, 0) != c.oracle(st)


# Cells that populations of two samples force to NA whatever the rows (W-4): D and H (a1-based variances
# of n = 2), ZnS at min_freq 2 (no site has 2 <= m <= n - 2), EHHS (fewer than 4 samples)
FORCED_NA_AT_TWO = ("D[", "H[", "Zns[", "EHHS[")


@pytest.mark.parametrize("name", ALL_CASES)
def test_oracle_text_is_informative(name):
    """At most a quarter of a case's printed statistic cells are NA / nan / inf / 0.00000.  Counted over
    every window and statistic, except: a tier list (T) is dealt out between short, empty and sparse
    windows on purpose, so its dense windows are counted; a gather case (G) is about windows of 0, 1 and
    2 segregating rows as well, so its other windows are counted; at 4 samples (W-4) the cells that
    populations of two force to NA are not counted."""
    c = we.case(name)
    windows, skip = None, ()
    if name.startswith("T-"):
        windows = set(c.wins[0:14:2])
    elif name.startswith("G-"):
        S = c.census(we.S_TREE)["S"].tolist()
        windows = {w for w, x in zip(c.wins, S) if x > 2}
        assert len(windows) == len(c.wins) - 3
    elif name == "W-4":
        assert [c.params.pop_n[i] for i in range(c.params.n_pops)] == [2, 2]
        skip = FORCED_NA_AT_TWO
    share = we.dull_share(c, windows, skip)
    print(f"{name}: dull cells {share:.3f}")
    assert share <= 0.25


@pytest.mark.parametrize("name", ALL_CASES)
def test_tree_jc_is_defined_where_it_runs(name):
    c = we.case(name)
    if any(st[0] == we.S_TREE and st[4] == 1 for st in c.stats):
        assert we.tree_jc_defined(c)
    else:
        assert name[0] in "WO"


# ---------------------------------------------------------------- GPU: the text against the oracle's
@pytest.mark.gpu
@pytest.mark.parametrize("name", T_CASES)
def test_segcap_tiers_match_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", P_CASES)
def test_bitplanes_past_segcap_match_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", G_CASES)
def test_bitplane_gather_matches_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", W_CASES)
def test_u16_wrap_at_65536_matches_oracle(gpu_lib, name):
    assert we.run_case(name) == 10


@pytest.mark.gpu
@pytest.mark.parametrize("name", H_CASES)
def test_nhaps_merge_matches_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", E_CASES)
def test_ehhs_ties_match_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", L_CASES)
def test_wall_partitions_match_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", Z_TWO + Z_MANY)
def test_zns_list_capacity_matches_oracle(gpu_lib, name):
    assert we.run_case(name) == 12


@pytest.mark.gpu
@pytest.mark.parametrize("name", R_CASES)
def test_r2_table_placement_matches_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", S_CASES)
def test_short_chains_match_oracle(gpu_lib, name):
    assert we.run_case(name) == 13


@pytest.mark.gpu
@pytest.mark.parametrize("name", O_CASES)
def test_outgroup_flip_matches_oracle(gpu_lib, name):
    assert we.run_case(name) == 2


# ---------------------------------------------------------------- GPU: the same paths on the bounds build
SNIPPET = r"""
import sys
sys.path[:0] = [{repo!r}, {tests!r}, {golden!r}]
import window_edges as we
from popbam_amd import _lib
assert _lib.load().pbg_build_info() == b"bounds"
out = []
for name in {names!r}:
    try:
        we.run_case(name)   # every text equals the oracle's; pbg_check returns 0 after every call
        out.append(name + ":ok")
    except (AssertionError, RuntimeError) as e:
        out.append(name + ":" + type(e).__name__ + " " + str(e)[:300].replace("\n", " ").replace("|", "/"))
print("|".join(out))
"""


@pytest.mark.gpu
def test_edges_on_the_bounds_build(gpu_lib):
    """Tier, wrap, nhaps and ZnS-capacity cases on the PBG_BOUNDS build (a child process with
    POPBAM_GPU_LIB, as test_bounds_build._run): the same text, and pbg_check returns 0 -- no store
    outside a window's pool slice, a ZnS list region or an omega / Wall list on any of these paths."""
    assert os.path.exists(BOUNDS_LIB), "build it with __graft_entry__.build() (make bounds)"
    env = dict(os.environ)
    env.pop("PBG_BOUNDS_SELFTEST", None)
    env["POPBAM_GPU_LIB"] = BOUNDS_LIB
    code = SNIPPET.format(repo=REPO, tests=os.path.join(REPO, "tests"), golden=os.path.join(REPO, "tests", "golden"),
                          names=BOUNDS_CASES)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].split("|") == [n + ":ok" for n in BOUNDS_CASES]


# ---------------------------------------------------------------- CPU: the founder goldens carry structure
@pytest.mark.parametrize("name,pop,n_pop", [("g19_founders24", "pa", 8), ("g20_founders64", "popA", 32)])
def test_founder_goldens_show_structure(name, pop, n_pop):
    """The reference's own text for the two golden cases simulated with founders: samples of the first
    population share haplotypes in most windows (K below its size), and Wall's B is positive somewhere."""
    import fixtures
    import harness
    cases = fixtures.load_case(name)["meta"]["cases"]

    def text(args):
        cs = next(c for c in cases if c["args"] == args)
        return fixtures.golden_text(name, cs["stdout"])
    k = [int(v) for (li, lb), v in harness.labelled_values(text(["haplo", "-w", "1"])).items() if lb == f"K[{pop}]:"]
    print(f"{name}: K[{pop}] per window {k} of {n_pop} samples")
    assert len(k) >= 4 and sum(2 <= x < n_pop for x in k) > len(k) // 2
    b = [v for (li, lb), v in harness.labelled_values(text(["ld", "-w", "1", "-o", "2"])).items() if lb.startswith("B[")]
    assert any(v.strip() != "NA" and float(v) > 0 for v in b)
