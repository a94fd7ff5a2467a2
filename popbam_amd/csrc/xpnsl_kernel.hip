// xpnsl_kernel.hip -- the cross-population nSL tract sums on gfx950 (XP-nSL, Szpiech et al. 2021), per
// window and population pair (pbg_window_xpnsl; no reference counterpart, DESIGN.md "XP-nSL").
//
// A chain is one (window, pair (i, j), i < j).  Its pooled sites are the window's segregating rows whose
// derived count m in pm_i | pm_j has 1 <= m <= n_i + n_j - 1, in row order, each read as its column
// x = types & (pm_i | pm_j): pbg_window_nsl's list for the single population pm_i | pm_j.  Side 0 is
// population i, side 1 population j.  A pair u < v of one side's samples agrees at site k when bits u and
// v of x_k are equal, whichever allele they share.  With l and r the runs of agreement through k, k - 1,
// ... and k, k + 1, ... over the pooled list, its tract length is L = l + r - 1, and sl[k][s] is the sum
// of L over side s's agreeing pairs.
//
// The structure is nsl_kernel.hip's: one wave per chain, `waves` chains per workgroup (4, 2 or 1 by the
// LDS plan), nothing shared between the waves, no workgroup barrier; the passes count, forward and
// backward; one last[p] per sample pair, both sides' pairs in one table (side 0's, then side 1's).
// Forward, last[p] is the last site at which pair p differed (-1 before the first); backward it is the
// mirror image from V.  Every agreeing pair is counted by both walks, so
// sl[k][s] = left + right - A_s with A_s = C(m_s, 2) + C(n_s - m_s, 2), the agreeing pairs at the site.
//
// There are no classes, so a side's sum over its agreeing pairs is its sum over all pairs less that over
// the differing ones, and the sum over all pairs needs no loop: with sumlast_s the sum of last[p] over
// the side (wave-uniform, int64) it is |C_s k - sumlast_s|.  Likewise the agreeing pairs still at the
// walk's start value are nedge_s less the differing ones that were.  So
//   - at a site where side s is monomorphic (m_s = 0 or n_s: every pair agrees, no last[p] moves) the
//     side's totals are |C_s k - sumlast_s| and nedge_s: no LDS traffic and no scan;
//   - at a site where it varies the lanes stride over its pairs, only the differing ones add (their
//     |k - last| and whether last was the start value) and move last to k; two wave sums per side give
//     the site's totals and the change of sumlast_s and nedge_s.
// A pooled list holds many sites at which one side is monomorphic (every site fixed in one population
// and variable in the other), which is what the shortcut is for.  All of it is integer and order-free:
// a lane sums at most ceil(7,875 / 64) = 124 distances below 2^31, so a lane's sum is below 2^38, the
// bound of the split scan (wave_sum38), and |sumlast_s| <= 7,875 * 2^31 < 2^44.  Two runs give the
// same bytes.
//
// The backward walk reads the sites back through row[] after a device-scope fence (which is why sl and
// cens need row), 64 at a time from the back, the next trip's loads issued before this trip's walk; a
// row index is checked against n_rows before the row is read.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_xpnsl = PBG_BUILD_KIND;   // pbg_build_info()
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

__device__ __forceinline__ uint64_t join(uint64_t a, uint64_t b) { return a | b; }
__device__ __forceinline__ M2 join(M2 a, M2 b) { return {a.lo | b.lo, a.hi | b.hi}; }

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

__device__ __forceinline__ int64_t choose2(int64_t n) { return n * (n - 1) / 2; }

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_xpnsl_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                           uint32_t n_win, XpnslArgs A) {
    using M = typename RowMask<RB>::T;
    using Q = QueuedRow<RB>;
    using QT = typename Q::T;
    constexpr int R = 16 / RB;
    extern __shared__ uint4 s_xpnsl[];
    const int np = P.npops, npairs = np * (np - 1) / 2, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t ch = (uint64_t)blockIdx.x * (uint64_t)A.waves + (uint64_t)wave;
    if (ch >= (uint64_t)n_win * (uint64_t)npairs) return;   // the whole wave
    // this wave's LDS: [queue bits 64 * R][queue rows 64 * R][last: pairs_max][uv: pairs_max][pos: 128]
    unsigned char *base = reinterpret_cast<unsigned char *>(s_xpnsl) + (size_t)wave * A.wave_bytes;
    QT *qx = reinterpret_cast<QT *>(base);
    int32_t *qrow = reinterpret_cast<int32_t *>(qx + 64 * R);
    int32_t *last = qrow + 64 * R;
    uint16_t *uv = reinterpret_cast<uint16_t *>(last + A.pairs_max);
    uint8_t *pos = reinterpret_cast<uint8_t *>(uv + ((A.pairs_max + 1) & ~1));

    const uint32_t w = (uint32_t)(ch / (uint64_t)npairs);
    int pi = 0, pj = (int)(ch - (uint64_t)w * (uint64_t)npairs);   // pair (pi, pj), pi < pj, lexicographic
    while (pj >= np - 1 - pi) {
        pj -= np - 1 - pi;
        ++pi;
    }
    pj += pi + 1;
    const int n0 = P.pop_n[pi], n1 = P.pop_n[pj], nn = n0 + n1, ms = A.max_sites;
    const M pm0 = pop_mask<M>(P, pi), pm1 = pop_mask<M>(P, pj), pmu = join(pm0, pm1);
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, lane);
    const size_t s0 = (size_t)ch * (size_t)ms;   // the chain's first slot
    int32_t *o_row = A.row ? A.row + s0 : nullptr, *o_m = A.m ? A.m + s0 * 2 : nullptr;
    int64_t *o_sl = A.sl ? A.sl + s0 * 2 : nullptr;
    int32_t *o_cens = A.cens ? A.cens + s0 * 2 : nullptr;

    // count
    uint32_t nv = 0;
    if (!win.empty)
        gather_rows_in_order<RB, 4>(
            rows, n_rows, win, lane,
            [&](M &t, bool, bool sg) {
                const int m = (int)pc(t & pmu);
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
        if (o_m) o_m[2 * (size_t)k] = o_m[2 * (size_t)k + 1] = 0;
        if (o_sl) o_sl[2 * (size_t)k] = o_sl[2 * (size_t)k + 1] = 0;
        if (o_cens) o_cens[2 * (size_t)k] = o_cens[2 * (size_t)k + 1] = 0;
    }
    if (!fits || V == 0) return;

    const int C0 = n0 * (n0 - 1) / 2, C1 = n1 * (n1 - 1) / 2, Pn = C0 + C1;   // 0 when both sides are one sample
    const bool walks = (o_sl || o_cens) && o_row;
    // a site's sum over the wave stays below 2^32 when every distance is at most V + 1: one scan
    const bool narrow = ((uint64_t)V + 1) * (uint64_t)(Pn > 0 ? Pn : 1) < (1ULL << 32);
    if (walks && Pn > 0) {
        if (!PBG_STORE_OK(A.err, Pn - 1, A.pairs_max, A.pairs_max, kErrPool)) return;   // wave-uniform
        // the pair table: each side's samples by ascending bit, then its pairs (u, v), u < v; side 0 first
        for (int l = lane; l < (RB == 16 ? 128 : 64); l += 64) {
            if (bit(pm0, l)) pos[rank_below(pm0, l)] = (uint8_t)l;
            else if (bit(pm1, l)) pos[n0 + rank_below(pm1, l)] = (uint8_t)l;
        }
        wave_sync();
        auto fill = [&](int n, int pos0, int pair0, int Cn) {
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
                uv[pair0 + p] = (uint16_t)(pos[pos0 + u] | (uint32_t)pos[pos0 + v] << 8);
                last[pair0 + p] = -1;
                if (p + 64 < Cn) advance(64);
            }
        };
        fill(n0, 0, 0, C0);
        fill(n1, n0, C0, C1);
        wave_sync();
    }

    // the walk's state per side, wave-uniform: the sum of last[] and the pairs still at the start value
    int64_t sum0 = -(int64_t)C0, sum1 = -(int64_t)C1;
    int32_t ne0 = C0, ne1 = C1;

    // one site of a walk against column x: per side the sum of |k - last| over its agreeing pairs and
    // those of them whose last is still `edge`; a differing pair moves last to k
    auto site = [&](const M &x, int k, int edge, uint64_t &t0, uint64_t &t1, uint32_t &c0, uint32_t &c1) {
        const int m0 = __builtin_amdgcn_readfirstlane((int)pc(x & pm0));
        const int m1 = __builtin_amdgcn_readfirstlane((int)pc(x & pm1));
#ifdef PBG_XPNSL_PLAIN   // an experiment switch: the timing variant without the shortcut
        const bool var0 = true, var1 = true;
#else
        const bool var0 = m0 > 0 && m0 < n0, var1 = m1 > 0 && m1 < n1;
#endif
        const bool fwd = edge < 0;
        const int64_t all0 = fwd ? (int64_t)C0 * k - sum0 : sum0 - (int64_t)C0 * k;
        const int64_t all1 = fwd ? (int64_t)C1 * k - sum1 : sum1 - (int64_t)C1 * k;
        uint64_t dd0 = 0, dd1 = 0;
        uint32_t de0 = 0, de1 = 0;
        if (var0 || var1) {
            uint64_t d0 = 0, d1 = 0;
            uint32_t e0 = 0, e1 = 0;
            // pair p is lane p % 64's at every site of both walks, whichever sides are walked, so
            // last[p] is only ever read and written by one lane and needs no wave_sync between sites
            const int lo = var0 ? 0 : C0, hi = var1 ? Pn : C0;
            for (int p = (lo & ~63) + lane; p < hi; p += 64) {
                if (p < lo) continue;
                const uint32_t e = uv[p];
                const int32_t la = last[p];
                if (bit(x, (int)(e & 255u)) != bit(x, (int)(e >> 8))) {
                    const uint32_t d = (uint32_t)(k > la ? k - la : la - k), at = la == edge ? 1u : 0u;
                    if (p < C0) {
                        d0 += d;
                        e0 += at;
                    } else {
                        d1 += d;
                        e1 += at;
                    }
                    last[p] = k;
                }
            }
            if (var0) {
                dd0 = narrow ? (uint64_t)wave_sum32((uint32_t)d0) : wave_sum38(d0);
                de0 = wave_sum32(e0);
            }
            if (var1) {
                dd1 = narrow ? (uint64_t)wave_sum32((uint32_t)d1) : wave_sum38(d1);
                de1 = wave_sum32(e1);
            }
        }
        t0 = (uint64_t)all0 - dd0;
        t1 = (uint64_t)all1 - dd1;
        c0 = (uint32_t)ne0 - de0;
        c1 = (uint32_t)ne1 - de1;
        sum0 += fwd ? (int64_t)dd0 : -(int64_t)dd0;
        sum1 += fwd ? (int64_t)dd1 : -(int64_t)dd1;
        ne0 -= (int32_t)de0;
        ne1 -= (int32_t)de1;
    };

    // forward
    int kbase = 0;   // wave-uniform: the sites before this trip
    stream_rows_in_order<RB, 4>(
        rows, n_rows, win, lane, qx, qrow,
        [&](M &t) -> bool {
            t = t & pmu;
            const int m = (int)pc(t);
            return m >= 1 && m <= nn - 1;
        },
        [&](int nq) {
            for (int j = lane; j < nq; j += 64)
                if (PBG_STORE_OK(A.err, kbase + j, ms, ms, kErrPool)) {
                    if (o_row) o_row[kbase + j] = qrow[j];
                    if (o_m) {
                        const M x = Q::get(qx[j]);
                        o_m[2 * (size_t)(kbase + j)] = (int32_t)pc(x & pm0);
                        o_m[2 * (size_t)(kbase + j) + 1] = (int32_t)pc(x & pm1);
                    }
                }
            if (walks)
                for (int c0 = 0; c0 < nq; c0 += 64) {
                    const int cnt = nq - c0 < 64 ? nq - c0 : 64;
                    uint64_t r0 = 0, r1 = 0;
                    uint32_t rc0 = 0, rc1 = 0;
                    for (int kk = 0; kk < cnt; ++kk) {
                        uint64_t t0, t1;
                        uint32_t tc0, tc1;
                        site(Q::get(qx[c0 + kk]), kbase + c0 + kk, -1, t0, t1, tc0, tc1);
                        if (lane == kk) {
                            r0 = t0;
                            r1 = t1;
                            rc0 = tc0;
                            rc1 = tc1;
                        }
                    }
                    const int k = kbase + c0 + lane;
                    if (lane < cnt && PBG_STORE_OK(A.err, k, ms, ms, kErrPool)) {
                        if (o_sl) {
                            o_sl[2 * (size_t)k] = (int64_t)r0;
                            o_sl[2 * (size_t)k + 1] = (int64_t)r1;
                        }
                        if (o_cens) {
                            o_cens[2 * (size_t)k] = (int32_t)rc0;
                            o_cens[2 * (size_t)k + 1] = (int32_t)rc1;
                        }
                    }
                }
            kbase += nq;
        });
    if (!walks) return;

    // backward
    __threadfence();   // row[] and the left sums, stored by other lanes of this wave
    for (int p = lane; p < Pn; p += 64) last[p] = V;
    sum0 = (int64_t)C0 * V;
    sum1 = (int64_t)C1 * V;
    ne0 = C0;
    ne1 = C1;
    auto fetch = [&](int k0) -> M {   // the column of site k0 + lane
        const int k = k0 + lane;
        if (k0 < 0 || k >= V) return M{};
        const int32_t r = load_fresh(o_row + k);
        if (r < 0 || (uint32_t)r >= n_rows) return M{};   // never: a row index this chain stored
        return load_row_bits<RB>(rows, r) & pmu;
    };
    int k0 = ((V - 1) / 64) * 64;
    M xc = fetch(k0);
    for (; k0 >= 0; k0 -= 64) {
        const int cnt = V - k0 < 64 ? V - k0 : 64;
        const M xn = fetch(k0 - 64);
        qx[lane] = Q::put(xc);
        wave_sync();
        uint64_t r0 = 0, r1 = 0;
        uint32_t rc0 = 0, rc1 = 0;
        for (int kk = cnt - 1; kk >= 0; --kk) {
            uint64_t t0, t1;
            uint32_t tc0, tc1;
            site(Q::get(qx[kk]), k0 + kk, V, t0, t1, tc0, tc1);
            if (lane == kk) {
                r0 = t0;
                r1 = t1;
                rc0 = tc0;
                rc1 = tc1;
            }
        }
        const int k = k0 + lane;
        if (lane < cnt && PBG_STORE_OK(A.err, k, ms, ms, kErrPool)) {
            if (o_sl) {
                const int64_t m0 = (int64_t)pc(xc & pm0), m1 = (int64_t)pc(xc & pm1);
                o_sl[2 * (size_t)k] = load_fresh(o_sl + 2 * (size_t)k) + (int64_t)r0 - choose2(m0) - choose2(n0 - m0);
                o_sl[2 * (size_t)k + 1] = load_fresh(o_sl + 2 * (size_t)k + 1) + (int64_t)r1 - choose2(m1) - choose2(n1 - m1);
            }
            if (o_cens) {
                o_cens[2 * (size_t)k] = load_fresh(o_cens + 2 * (size_t)k) + (int32_t)rc0;
                o_cens[2 * (size_t)k + 1] = load_fresh(o_cens + 2 * (size_t)k + 1) + (int32_t)rc1;
            }
        }
        wave_sync();   // the next trip's queue
        xc = xn;
    }
}

hipError_t launch_window_xpnsl(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win, XpnslArgs A,
                               hipStream_t stream) {
    const int npairs = P.npops * (P.npops - 1) / 2;
    if (n_win == 0 || npairs == 0) return hipSuccess;
    // both sides' pairs share a chain's table; the populations are disjoint and hold at most 126 samples,
    // so the largest C(n_i, 2) + C(n_j, 2) is at most C(126, 2), pbg_window_nsl's own worst case
    A.pairs_max = 1;
    for (int i = 0; i < P.npops; ++i)
        for (int j = i + 1; j < P.npops; ++j) {
            const int c = P.pop_n[i] * (P.pop_n[i] - 1) / 2 + P.pop_n[j] * (P.pop_n[j] - 1) / 2;
            A.pairs_max = c > A.pairs_max ? c : A.pairs_max;
        }
    const size_t wb = nsl_wave_bytes(rb, A.pairs_max);   // the same per-wave layout
    if (wb > 64 * 1024) return hipErrorInvalidValue;   // never: 7,875 pairs take 48,672 bytes
    A.wave_bytes = (uint32_t)wb;
    A.waves = 4 * wb <= 64 * 1024 ? 4 : 2 * wb <= 64 * 1024 ? 2 : 1;
    const uint64_t chains = (uint64_t)n_win * (uint64_t)npairs;
    const dim3 g((uint32_t)((chains + A.waves - 1) / A.waves)), b(64 * A.waves);
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_xpnsl_kernel<decltype(RB)::value>, g, b, (size_t)A.waves * wb, stream, P, rows, n_rows,
                           n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
