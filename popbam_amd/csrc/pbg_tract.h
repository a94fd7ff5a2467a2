// pbg_tract.h -- the tract walk that nsl_kernel.hip and xpnsl_kernel.hip share: per chain a list of
// sites in row order, one int32 per sample pair, and two walks over the list that sum, site by site,
// how far back (forward) each agreeing pair last differed.  The statistic -- which rows are sites,
// which pairs count, what is summed -- is a policy (below); the mechanics are here, once.
//
// One wave per chain, `waves` chains per workgroup (tract_plan picks 4, 2 or 1 so that the launch's LDS
// stays within 64 KiB), nothing shared between the waves and no workgroup barrier.  Per wave, in LDS
// (TractLds): the row queue of the ordered stream (pbg_rows.h), last[] and the (u, v) table of the
// chain's pairs as sample bit positions.  A chain takes three passes:
//   count     the stream with nothing kept: V.  A count-only call (max_sites = 0) and a chain with
//             V > max_sites stop here, every slot written as unused;
//   forward   the stream again: row[] and m[] from the queue, then site by site (a wave-uniform LDS read
//             of the column) the policy's site(); its per-site totals are wave-uniform, parked in the
//             lane of the site's slot and stored 64 sites at a time.  last[p] is the last site at which
//             pair p differed, -1 before the first;
//   backward  64 sites at a time from the back, the mirror image from last[p] = V: each lane reads its
//             site's row index back from row[] after a device-scope fence (which is why sl and cens need
//             row), then the row itself, the next trip's loads issued before this trip's walk; a row
//             index is checked against n_rows before the row is read.
// Integers only and order-free sums, so two runs give the same bytes.
//
// The policy of a statistic (NslWalk, XpnslWalk) supplies:
//   kM, Tot             the ints of m[] per site; the per-site totals site() returns
//   pm, is_site(x)      the pooled sample mask; whether a segregating row, masked to x, is a site
//   Pn, pairs(L)        the chain's pairs; their table, through tract_pairs
//   store_m(o, x)       m[] of a site
//   start(V, edge)      a walk begins (edge = -1 forward, V backward)
//   site(x, k, edge)    one site of a walk against column x: moves last[] and returns the totals
//   store_fwd(O, k, r)  the raw left sums
//   store_bwd(O, k, r, x)  left + right less the correction, cens in the statistic's own form
#pragma once
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {

// the sum of v < 2^38 over the wave, wave-uniform: two integer scans of 20- and 18-bit halves
__device__ __forceinline__ uint64_t wave_sum38(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_s((uint32_t)v & 0xFFFFFu), 63);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_s((uint32_t)(v >> 20)), 63);
    return ((uint64_t)hi << 20) + lo;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_s(v), 63);
}

// the number of set bits of pm below bit l
__device__ __forceinline__ int rank_below(uint64_t pm, int l) { return (int)pc(pm & ((1ULL << l) - 1)); }
__device__ __forceinline__ int rank_below(M2 pm, int l) {
    return l < 64 ? rank_below(pm.lo, l) : (int)pc(pm.lo) + rank_below(pm.hi, l - 64);
}

// row ri (< n_rows) alone: its sample bits
template <int RB>
__device__ __forceinline__ typename RowMask<RB>::T load_row_bits(const void *rows, int64_t ri) {
    uint4 q = make_uint4(0, 0, 0, 0);
    if constexpr (RB == 16) {
        q = reinterpret_cast<const uint4 *>(rows)[ri];
    } else if constexpr (RB == 8) {
        const uint64_t v = reinterpret_cast<const uint64_t *>(rows)[ri];
        q.x = (uint32_t)v;
        q.y = (uint32_t)(v >> 32);
    } else if constexpr (RB == 4) {
        q.x = reinterpret_cast<const uint32_t *>(rows)[ri];
    } else {
        q.x = reinterpret_cast<const uint16_t *>(rows)[ri];
    }
    typename RowMask<RB>::T t;
    bool cnt, sg;
    row_in_word<RB>(q, 0, t, cnt, sg);
    return t;
}

// a load that sees what other lanes of this wave stored before the fence
template <class T>
__device__ __forceinline__ T load_fresh(const T *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__host__ __device__ __forceinline__ int64_t choose2(int64_t n) { return n * (n - 1) / 2; }

// a wave's LDS: [queue bits 64 * R][queue rows 64 * R][last: pairs_max][uv: pairs_max][pos: 128]
template <int RB>
struct TractLds {
    using QT = typename QueuedRow<RB>::T;
    static constexpr int R = 16 / RB;
    QT *qx;
    int32_t *qrow, *last;
    uint16_t *uv;
    uint8_t *pos;
    __device__ __forceinline__ TractLds(unsigned char *base, int pairs_max)
        : qx(reinterpret_cast<QT *>(base)), qrow(reinterpret_cast<int32_t *>(qx + 64 * R)), last(qrow + 64 * R),
          uv(reinterpret_cast<uint16_t *>(last + pairs_max)), pos(reinterpret_cast<uint8_t *>(uv + ((pairs_max + 1) & ~1))) {}
};
// its size
inline size_t nsl_wave_bytes(int rb, int pairs_max) {
    const size_t R = 16 / (size_t)rb, qt = rb == 16 ? 16 : rb == 8 ? 8 : 4;
    const size_t b = 64 * R * (qt + 4) + (size_t)pairs_max * 4 + (((size_t)pairs_max + 1) & ~(size_t)1) * 2 + 128;
    return (b + 15) & ~(size_t)15;
}

// The launch plan of `chains` chains whose largest pair table has pairs_max entries: the LDS per wave,
// the waves per workgroup and the grid.  Fills A's launcher fields; false when one wave cannot fit.
struct TractPlan {
    dim3 grid, block;
    size_t lds;
};
inline bool tract_plan(int rb, int pairs_max, uint64_t chains, TractArgs &A, TractPlan &plan) {
    const size_t wb = nsl_wave_bytes(rb, pairs_max);
    if (wb > 64 * 1024) return false;   // never: the 7,875 pairs of 126 samples take 48,672 bytes
    A.pairs_max = pairs_max;
    A.wave_bytes = (uint32_t)wb;
    A.waves = 4 * wb <= 64 * 1024 ? 4 : 2 * wb <= 64 * 1024 ? 2 : 1;
    plan = {dim3((uint32_t)((chains + A.waves - 1) / A.waves)), dim3(64 * A.waves), (size_t)A.waves * wb};
    return true;
}

// a chain's slots of the per-site arrays (null where the caller wants none)
struct TractOut {
    int32_t *row, *m;
    int64_t *sl;
    int32_t *cens;
};

// the pair table of n samples, the set bits of pm by ascending bit: their positions from pos[pos0] on,
// then pair p = (u, v), u < v, at uv[pair0 + p], last[] at the forward walk's start
template <int RB, class M>
__device__ __forceinline__ void tract_pairs(const TractLds<RB> &L, int lane, const M &pm, int n, int pos0, int pair0) {
    for (int l = lane; l < (RB == 16 ? 128 : 64); l += 64)
        if (bit(pm, l)) L.pos[pos0 + rank_below(pm, l)] = (uint8_t)l;
    wave_sync();
    const int Cn = n * (n - 1) / 2;
    int u = 0, v = 1;
    auto advance = [&](int d) {   // d pairs on; the target exists
        while (d > 0) {
            const int room = n - 1 - v;
            if (d <= room) {
                v += d;
                d = 0;
            } else {
                d -= room + 1;
                ++u;
                v = u + 1;
            }
        }
    };
    if (lane < Cn) advance(lane);
    for (int p = lane; p < Cn; p += 64) {
        L.uv[pair0 + p] = (uint16_t)(L.pos[pos0 + u] | (uint32_t)L.pos[pos0 + v] << 8);
        L.last[pair0 + p] = -1;
        if (p + 64 < Cn) advance(64);
    }
}

// the forward walk: row[], m[] and, when the chain walks, the policy's left sums
template <int RB, class W>
__device__ __forceinline__ void tract_forward(const void *rows, uint32_t n_rows, const WindowRows &win, int lane, int *err,
                                              int ms, const TractLds<RB> &L, const TractOut &O, bool walks, W &pol) {
    using M = typename RowMask<RB>::T;
    using Q = QueuedRow<RB>;
    int kbase = 0;   // wave-uniform: the sites before this trip
    stream_rows_in_order<RB, 4>(
        rows, n_rows, win, lane, L.qx, L.qrow,
        [&](M &t) -> bool {
            t = t & pol.pm;
            return pol.is_site(t);
        },
        [&](int nq) {
            for (int j = lane; j < nq; j += 64)
                if (PBG_STORE_OK(err, kbase + j, ms, ms, kErrPool)) {
                    if (O.row) O.row[kbase + j] = L.qrow[j];
                    if (O.m) pol.store_m(O.m + (size_t)W::kM * (kbase + j), Q::get(L.qx[j]));
                }
            if (walks)
                for (int c0 = 0; c0 < nq; c0 += 64) {
                    const int cnt = nq - c0 < 64 ? nq - c0 : 64;
                    typename W::Tot r{};
                    for (int kk = 0; kk < cnt; ++kk) {
                        const typename W::Tot t = pol.site(Q::get(L.qx[c0 + kk]), kbase + c0 + kk, -1);
                        if (lane == kk) r = t;
                    }
                    const int k = kbase + c0 + lane;
                    if (lane < cnt && PBG_STORE_OK(err, k, ms, ms, kErrPool)) pol.store_fwd(O, k, r);
                }
            kbase += nq;
        });
}

// the backward walk over the V sites the forward walk stored
template <int RB, class W>
__device__ __forceinline__ void tract_backward(const void *rows, uint32_t n_rows, int lane, int *err, int ms, int V,
                                               const TractLds<RB> &L, const TractOut &O, W &pol) {
    using M = typename RowMask<RB>::T;
    using Q = QueuedRow<RB>;
    __threadfence();   // row[] and the left sums, stored by other lanes of this wave
    for (int p = lane; p < pol.Pn; p += 64) L.last[p] = V;
    pol.start(V, V);
    auto fetch = [&](int k0) -> M {   // the column of site k0 + lane
        const int k = k0 + lane;
        if (k0 < 0 || k >= V) return M{};
        const int32_t r = load_fresh(O.row + k);
        if (r < 0 || (uint32_t)r >= n_rows) return M{};   // never: a row index this chain stored
        return load_row_bits<RB>(rows, r) & pol.pm;
    };
    int k0 = ((V - 1) / 64) * 64;
    M xc = fetch(k0);
    for (; k0 >= 0; k0 -= 64) {
        const int cnt = V - k0 < 64 ? V - k0 : 64;
        const M xn = fetch(k0 - 64);
        L.qx[lane] = Q::put(xc);
        wave_sync();
        typename W::Tot r{};
        for (int kk = cnt - 1; kk >= 0; --kk) {
            const typename W::Tot t = pol.site(Q::get(L.qx[kk]), k0 + kk, V);
            if (lane == kk) r = t;
        }
        const int k = k0 + lane;
        if (lane < cnt && PBG_STORE_OK(err, k, ms, ms, kErrPool)) pol.store_bwd(O, k, r, xc);
        wave_sync();   // the next trip's queue
        xc = xn;
    }
}

// chain ch of a launch: count, the unused slots, the pair table and the two walks
template <int RB, class W>
__device__ __forceinline__ void tract_chain(const void *rows, uint32_t n_rows, const WindowRows &win, int lane,
                                            const TractArgs &A, uint64_t ch, const TractLds<RB> &L, W &pol) {
    using M = typename RowMask<RB>::T;
    const int ms = A.max_sites;
    const size_t s0 = (size_t)ch * (size_t)ms;   // the chain's first slot
    const TractOut O{A.row ? A.row + s0 : nullptr, A.m ? A.m + s0 * W::kM : nullptr, A.sl ? A.sl + s0 * 2 : nullptr,
                     A.cens ? A.cens + s0 * 2 : nullptr};

    // count
    uint32_t nv = 0;
    if (!win.empty)
        gather_rows_in_order<RB, 4>(
            rows, n_rows, win, lane,
            [&](M &t, bool, bool sg) {
                nv += (sg && pol.is_site(t & pol.pm)) ? 1u : 0u;
                return false;
            },
            [&](uint32_t, const M &, int64_t) {}, [&](uint32_t) {});
    const int V = (int)wave_sum32(nv);
    if (lane == 0 && A.n_var) A.n_var[ch] = V;
    if (ms == 0) return;
    const bool fits = V <= ms;
    for (int k = (fits ? V : 0) + lane; k < ms; k += 64) {   // the unused slots
        if (O.row) O.row[k] = -1;
        if (O.m)
            for (int c = 0; c < W::kM; ++c) O.m[(size_t)W::kM * k + c] = 0;
        if (O.sl) O.sl[2 * (size_t)k] = O.sl[2 * (size_t)k + 1] = 0;
        if (O.cens) O.cens[2 * (size_t)k] = O.cens[2 * (size_t)k + 1] = 0;
    }
    if (!fits || V == 0) return;

    const bool walks = (O.sl || O.cens) && O.row;
    if (walks && pol.Pn > 0) {
        if (!PBG_STORE_OK(A.err, pol.Pn - 1, A.pairs_max, A.pairs_max, kErrPool)) return;   // wave-uniform
        pol.pairs(L);
        wave_sync();
    }
    pol.start(V, -1);
    tract_forward<RB>(rows, n_rows, win, lane, A.err, ms, L, O, walks, pol);
    if (walks) tract_backward<RB>(rows, n_rows, lane, A.err, ms, V, L, O, pol);
}

}  // namespace pbg
