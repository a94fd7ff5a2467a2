// nsl_kernel.hip -- the per-site nSL tract sums on gfx950 (Ferrer-Admetlla et al. 2014), per window and
// population (pbg_window_nsl; no reference counterpart, DESIGN.md "nSL").
//
// A chain is one (window, population).  Its variable sites are pbg_window_rmin's at min_freq = 1: the
// window's segregating rows whose derived count m in the population has 1 <= m <= n - 1, in row order,
// each read as its column x = types & pm.  A pair u < v of the population's samples agrees at site k
// when bits u and v of x_k are equal; its class is the shared bit.  With l and r the numbers of
// consecutive sites k, k - 1, ... and k, k + 1, ... at which the pair agrees, its tract length is
// L = l + r - 1, and sl[k][c] is the sum of L over the pairs that agree at k with class c.
//
// L splits into two walks that need one integer per pair and no list of sites.  Forward, last[p] is
// the last site at which pair p differed (-1 before the first): an agreeing pair adds k - last[p] = l
// to its class's sum and counts as censored on the left when last[p] is still -1; a differing pair
// sets last[p] = k.  Backward is the mirror image from last[p] = V.  Every agreeing pair is counted in
// both walks, so sl[k][c] = left + right - P_c with P_0 = C(n - m, 2) and P_1 = C(m, 2).
//
// One wave per chain, `waves` chains per workgroup (the host picks 4, 2 or 1 so that the launch's LDS
// stays within 64 KiB), nothing shared between the waves and no workgroup barrier.  Per wave, in LDS:
// the row queue of the ordered stream (pbg_rows.h), last[] and the (u, v) table of the population's
// pairs as sample bit positions.  A chain takes three passes:
//   count     the stream with nothing kept: V.  A count-only call (max_sites = 0) and a chain with
//             V > max_sites stop here, every slot written as unused;
//   forward   the stream again: row[] and m[] from the queue, then site by site (a wave-uniform LDS read
//             of the column) the lanes stride over the pairs; the three per-site totals are wave sums
//             (DPP scans of integer halves, order-free), parked in the lane of the site's slot and
//             stored 64 sites at a time;
//   backward  64 sites at a time from the back: each lane reads its site's row index back from row[]
//             (which is why sl and cens need row), then the row itself, the next trip's loads issued
//             before this trip's walk; the same pair loop downwards; sl = left + right - P_c.
// Integers only, so two runs give the same bytes.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_nsl = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

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

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_nsl_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                         uint32_t n_win, NslArgs A) {
    using M = typename RowMask<RB>::T;
    using Q = QueuedRow<RB>;
    using QT = typename Q::T;
    constexpr int R = 16 / RB;
    extern __shared__ uint4 s_nsl[];
    const int np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t ch = (uint64_t)blockIdx.x * (uint64_t)A.waves + (uint64_t)wave;
    if (ch >= (uint64_t)n_win * (uint64_t)np) return;   // the whole wave
    // this wave's LDS: [queue bits 64 * R][queue rows 64 * R][last: pairs_max][uv: pairs_max][pos: 128]
    unsigned char *base = reinterpret_cast<unsigned char *>(s_nsl) + (size_t)wave * A.wave_bytes;
    QT *qx = reinterpret_cast<QT *>(base);
    int32_t *qrow = reinterpret_cast<int32_t *>(qx + 64 * R);
    int32_t *last = qrow + 64 * R;
    uint16_t *uv = reinterpret_cast<uint16_t *>(last + A.pairs_max);
    uint8_t *pos = reinterpret_cast<uint8_t *>(uv + ((A.pairs_max + 1) & ~1));

    const uint32_t w = (uint32_t)(ch / (uint64_t)np);
    const int i = (int)(ch - (uint64_t)w * (uint64_t)np);
    const int nn = P.pop_n[i], ms = A.max_sites;
    const M pm = pop_mask<M>(P, i);
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, lane);
    const size_t s0 = (size_t)ch * (size_t)ms;   // the chain's first slot
    int32_t *o_row = A.row ? A.row + s0 : nullptr, *o_m = A.m ? A.m + s0 : nullptr;
    int64_t *o_sl = A.sl ? A.sl + s0 * 2 : nullptr;
    int32_t *o_cens = A.cens ? A.cens + s0 * 2 : nullptr;

    // count
    uint32_t nv = 0;
    if (!win.empty)
        gather_rows_in_order<RB, 4>(
            rows, n_rows, win, lane,
            [&](M &t, bool, bool sg) {
                const int m = (int)pc(t & pm);
                nv += (sg && m >= 1 && m <= nn - 1) ? 1u : 0u;
                return false;
            },
            [&](uint32_t, const M &, int64_t) {}, [&](uint32_t) {});
    const int V = (int)wave_sum32(nv);
    if (lane == 0 && A.n_var) A.n_var[ch] = V;
    if (ms == 0) return;
    const bool fits = V <= ms;
    for (int k = (fits ? V : 0) + lane; k < ms; k += 64) {   // the unused slots
        if (o_row) o_row[k] = -1;
        if (o_m) o_m[k] = 0;
        if (o_sl) o_sl[2 * (size_t)k] = o_sl[2 * (size_t)k + 1] = 0;
        if (o_cens) o_cens[2 * (size_t)k] = o_cens[2 * (size_t)k + 1] = 0;
    }
    if (!fits || V == 0) return;

    const int Pn = nn * (nn - 1) / 2;   // >= 1: a variable site needs two samples
    const bool walks = (o_sl || o_cens) && o_row;
    if (walks) {
        if (!PBG_STORE_OK(A.err, Pn - 1, A.pairs_max, A.pairs_max, kErrPool)) return;   // wave-uniform
        // the pair table: the population's samples by ascending bit, then pair p = (u, v), u < v
        for (int l = lane; l < (RB == 16 ? 128 : 64); l += 64)
            if (bit(pm, l)) pos[rank_below(pm, l)] = (uint8_t)l;
        wave_sync();
        int u = 0, v = 1;
        auto advance = [&](int d) {   // d pairs on; the target exists
            while (d > 0) {
                const int room = nn - 1 - v;
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
        if (lane < Pn) advance(lane);
        for (int p = lane; p < Pn; p += 64) {
            uv[p] = (uint16_t)(pos[u] | (uint32_t)pos[v] << 8);
            last[p] = -1;
            if (p + 64 < Pn) advance(64);
        }
        wave_sync();
    }

    // one site of a walk: the lanes' pairs against column x; an agreeing pair adds |k - last| to its
    // class and counts as censored while last is still `edge`, a differing pair moves last to k
    auto site = [&](const M &x, int k, int edge, uint64_t &t0, uint64_t &t1, uint32_t &tc) {
        uint64_t a0 = 0, a1 = 0;
        uint32_t ce = 0;
        for (int p = lane; p < Pn; p += 64) {
            const uint32_t e = uv[p];
            const int32_t la = last[p];
            const uint32_t a = bit(x, (int)(e & 255u)), b = bit(x, (int)(e >> 8));
            if (a == b) {
                const uint32_t d = (uint32_t)(k > la ? k - la : la - k);
                if (a) a1 += d;
                else a0 += d;
                ce += la == edge ? 1u : 0u;
            } else {
                last[p] = k;
            }
        }
        t0 = wave_sum38(a0);
        t1 = wave_sum38(a1);
        tc = wave_sum32(ce);
    };

    // forward
    int kbase = 0;   // wave-uniform: the sites before this trip
    stream_rows_in_order<RB, 4>(
        rows, n_rows, win, lane, qx, qrow,
        [&](M &t) -> bool {
            t = t & pm;
            const int m = (int)pc(t);
            return m >= 1 && m <= nn - 1;
        },
        [&](int nq) {
            for (int j = lane; j < nq; j += 64)
                if (PBG_STORE_OK(A.err, kbase + j, ms, ms, kErrPool)) {
                    if (o_row) o_row[kbase + j] = qrow[j];
                    if (o_m) o_m[kbase + j] = (int32_t)pc(Q::get(qx[j]));
                }
            if (walks)
                for (int c0 = 0; c0 < nq; c0 += 64) {
                    const int cnt = nq - c0 < 64 ? nq - c0 : 64;
                    uint64_t r0 = 0, r1 = 0;
                    uint32_t rc = 0;
                    for (int kk = 0; kk < cnt; ++kk) {
                        uint64_t t0, t1;
                        uint32_t tc;
                        site(Q::get(qx[c0 + kk]), kbase + c0 + kk, -1, t0, t1, tc);
                        if (lane == kk) {
                            r0 = t0;
                            r1 = t1;
                            rc = tc;
                        }
                    }
                    const int k = kbase + c0 + lane;
                    if (lane < cnt && PBG_STORE_OK(A.err, k, ms, ms, kErrPool)) {
                        if (o_sl) {
                            o_sl[2 * (size_t)k] = (int64_t)r0;
                            o_sl[2 * (size_t)k + 1] = (int64_t)r1;
                        }
                        if (o_cens) o_cens[2 * (size_t)k] = (int32_t)rc;
                    }
                }
            kbase += nq;
        });
    if (!walks) return;

    // backward
    __threadfence();   // row[] and the left sums, stored by other lanes of this wave
    for (int p = lane; p < Pn; p += 64) last[p] = V;
    auto fetch = [&](int k0) -> M {   // the column of site k0 + lane
        const int k = k0 + lane;
        if (k0 < 0 || k >= V) return M{};
        const int32_t r = load_fresh(o_row + k);
        if (r < 0 || (uint32_t)r >= n_rows) return M{};   // never: a row index this chain stored
        return load_row_bits<RB>(rows, r) & pm;
    };
    int k0 = ((V - 1) / 64) * 64;
    M xc = fetch(k0);
    for (; k0 >= 0; k0 -= 64) {
        const int cnt = V - k0 < 64 ? V - k0 : 64;
        const M xn = fetch(k0 - 64);
        qx[lane] = Q::put(xc);
        wave_sync();
        uint64_t r0 = 0, r1 = 0;
        uint32_t rc = 0;
        for (int kk = cnt - 1; kk >= 0; --kk) {
            uint64_t t0, t1;
            uint32_t tc;
            site(Q::get(qx[kk]), k0 + kk, V, t0, t1, tc);
            if (lane == kk) {
                r0 = t0;
                r1 = t1;
                rc = tc;
            }
        }
        const int k = k0 + lane;
        if (lane < cnt && PBG_STORE_OK(A.err, k, ms, ms, kErrPool)) {
            if (o_sl) {
                const int64_t m = (int64_t)pc(xc), z = (int64_t)nn - m;
                o_sl[2 * (size_t)k] = load_fresh(o_sl + 2 * (size_t)k) + (int64_t)r0 - z * (z - 1) / 2;
                o_sl[2 * (size_t)k + 1] = load_fresh(o_sl + 2 * (size_t)k + 1) + (int64_t)r1 - m * (m - 1) / 2;
            }
            if (o_cens) o_cens[2 * (size_t)k + 1] = (int32_t)rc;
        }
        wave_sync();   // the next trip's queue
        xc = xn;
    }
}

size_t nsl_wave_bytes(int rb, int pairs_max) {
    const size_t R = 16 / (size_t)rb, qt = rb == 16 ? 16 : rb == 8 ? 8 : 4;
    const size_t b = 64 * R * (qt + 4) + (size_t)pairs_max * 4 + (((size_t)pairs_max + 1) & ~(size_t)1) * 2 + 128;
    return (b + 15) & ~(size_t)15;
}

hipError_t launch_window_nsl(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win, NslArgs A,
                             hipStream_t stream) {
    if (n_win == 0) return hipSuccess;
    int nmax = 2;
    for (int i = 0; i < P.npops; ++i) nmax = P.pop_n[i] > nmax ? P.pop_n[i] : nmax;
    A.pairs_max = nmax * (nmax - 1) / 2;
    const size_t wb = nsl_wave_bytes(rb, A.pairs_max);
    if (wb > 64 * 1024) return hipErrorInvalidValue;   // never: 126 samples take 48,672 bytes
    A.wave_bytes = (uint32_t)wb;
    A.waves = 4 * wb <= 64 * 1024 ? 4 : 2 * wb <= 64 * 1024 ? 2 : 1;
    const uint64_t chains = (uint64_t)n_win * (uint64_t)P.npops;
    const dim3 g((uint32_t)((chains + A.waves - 1) / A.waves)), b(64 * A.waves);
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_nsl_kernel<decltype(RB)::value>, g, b, (size_t)A.waves * wb, stream, P, rows, n_rows, n_win,
                           A);
    });
    return hipGetLastError();
}

}  // namespace pbg
