// rmin_kernel.hip -- Hudson and Kaplan's Rm on gfx950: the minimum number of recombination events the
// four-gamete test implies, and the intervals that witness them, per window and population
// (pbg_window_rmin; no reference counterpart, DESIGN.md "Rmin").
//
// A chain is one (window, population).  Its variable sites are decay's and ZnS's: the window's
// segregating rows whose derived count m in the population has min_freq <= m <= n - min_freq, in row
// order, each read as its column x = types & pm.  Sites a < b are incompatible when x_a & x_b,
// x_a & ~x_b, ~x_a & x_b and ~x_a & ~x_b all have a sample of the population.  Walking b upwards, a
// site that is incompatible with a site at or after the right end of the last chosen interval closes
// the interval (nearest such site, b); the number of intervals is Rm.
//
// The walk keeps no list of sites.  Between two cuts the sites seen are pairwise compatible (a later
// one would have cut), so their columns are splits of one tree on the population's n leaves: up to
// complement at most n - 3 distinct ones that are no singletons, and singletons (m = 1 or n - 1) are
// never incompatible with anything.  The state of a chain is therefore at most n - 3 entries
// (column, last row seen with this column or its complement) and the count: one entry per lane up to
// 62 samples (2-, 4- and 8-byte rows), two per lane for 16-byte rows (123 entries at 126 samples),
// all in registers.
//
// One wave per chain, four chains per workgroup, nothing shared between the waves and no workgroup
// barrier.  The wave streams its window's rows in order (pbg_rows.h) into an LDS queue of its own,
// then takes the queue site by site: a wave-uniform LDS read, four ANDs per entry, one ballot.  A cut
// takes the maximum of the incompatible entries' last rows over the wave and restarts the list with
// the cutting site; otherwise an equal or complementary entry has its row refreshed, or the column is
// appended.  Integers only, so two runs give the same bytes.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_rmin = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_rmin_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                          uint32_t n_win, RminArgs A) {
    using M = typename RowMask<RB>::T;
    using Q = QueuedRow<RB>;
    constexpr int R = 16 / RB;
    constexpr int S = RB == 16 ? 2 : 1;   // list entries per lane: n - 3 <= 64 * S
    __shared__ typename Q::T s_x[kRminWaves][64 * R];
    __shared__ int32_t s_row[kRminWaves][64 * R];
    const int np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t ch = (uint64_t)blockIdx.x * kRminWaves + (uint64_t)wave;
    if (ch >= (uint64_t)n_win * (uint64_t)np) return;   // the whole wave
    const uint32_t w = (uint32_t)(ch / (uint64_t)np);
    const int i = (int)(ch - (uint64_t)w * (uint64_t)np);
    const int nn = P.pop_n[i], mf = A.min_freq, max_cuts = A.max_cuts;
    const M pm = pop_mask<M>(P, i);
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, lane);
    int32_t *cuts = A.cuts ? A.cuts + (size_t)ch * (size_t)max_cuts * 2 : nullptr;

    M lx[S];          // the list: entry s * 64 + lane is valid below cnt
    int32_t lrow[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        lx[s] = M{};
        lrow[s] = -1;
    }
    int cnt = 0, rmin = 0;    // wave-uniform
    uint32_t nv = 0;          // this lane's variable sites
    const bool walks = nn >= 4;   // fewer than four samples cannot show four gametes

    if (!win.empty)
        stream_rows_in_order<RB, 4>(
            rows, n_rows, win, lane, s_x[wave], s_row[wave],
            [&](M &t) -> bool {
                t = t & pm;
                const int m = (int)pc(t);
                if (m < mf || m > nn - mf) return false;
                ++nv;
                return walks && m > 1 && m < nn - 1;   // a singleton counts and is never queued
            },
            [&](int nq) {
                for (int k = 0; k < nq; ++k) {
                    const M x = Q::get(s_x[wave][k]);
                    const int32_t row = s_row[wave][k];
                    const M nx = ~x & pm;
                    bool inc = false, same[S];
                    int32_t lr = -1;
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const bool valid = s * 64 + lane < cnt;
                        const M e = lx[s], ne = ~e & pm;
                        const bool bad = valid && nonzero(e & x) && nonzero(e & nx) && nonzero(ne & x) && nonzero(ne & nx);
                        inc |= bad;
                        if (bad && lrow[s] > lr) lr = lrow[s];
                        same[s] = valid && (e == x || e == nx);
                    }
                    if (__ballot(inc)) {   // wave-uniform from here
                        const int32_t left = wave_max(lr);
                        if (lane == 0) {
                            if (cuts && rmin < max_cuts) {
                                cuts[(size_t)rmin * 2] = left;
                                cuts[(size_t)rmin * 2 + 1] = row;
                            }
                            lx[0] = x;
                            lrow[0] = row;
                        }
                        ++rmin;
                        cnt = 1;
                        continue;
                    }
                    bool any = false;
#pragma unroll
                    for (int s = 0; s < S; ++s) any |= same[s];
                    if (__ballot(any)) {
#pragma unroll
                        for (int s = 0; s < S; ++s)
                            if (same[s]) lrow[s] = row;
                    } else if (cnt < 64 * S) {
#pragma unroll
                        for (int s = 0; s < S; ++s)
                            if (s * 64 + lane == cnt) {
                                lx[s] = x;
                                lrow[s] = row;
                            }
                        ++cnt;
                    } else if (lane == 0) {
                        atomicOr(A.err, 4);   // more splits than a tree has: never written past the list
                    }
                }
            });

    const uint32_t nvar = (uint32_t)__builtin_amdgcn_readlane((int)wave_incl_scan_s(nv), 63);
    if (lane == 0) {
        if (A.rmin) A.rmin[ch] = rmin;
        if (A.n_var) A.n_var[ch] = (int32_t)nvar;
    }
    if (cuts)
        for (int k = (rmin < max_cuts ? rmin : max_cuts) + lane; k < max_cuts; k += 64) {
            cuts[(size_t)k * 2] = -1;
            cuts[(size_t)k * 2 + 1] = -1;
        }
}

hipError_t launch_window_rmin(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                              const RminArgs &A, hipStream_t stream) {
    if (n_win == 0) return hipSuccess;
    const uint64_t chains = (uint64_t)n_win * (uint64_t)P.npops;
    const dim3 g((uint32_t)((chains + kRminWaves - 1) / kRminWaves)), b(64 * kRminWaves);
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_rmin_kernel<decltype(RB)::value>, g, b, 0, stream, P, rows, n_rows, n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
