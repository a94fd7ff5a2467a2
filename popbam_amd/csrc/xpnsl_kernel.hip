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
// The walk itself -- one wave per chain, the passes count, forward and backward, one last[p] per sample
// pair, the LDS and the launch plan -- is pbg_tract.h's; both sides' pairs share the table (side 0's,
// then side 1's).  Forward, last[p] is the last site at which pair p differed (-1 before the first);
// backward it is the mirror image from V.  Every agreeing pair is counted by both walks, so
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
#include "pbg_common.h"
#include "pbg_rows.h"
#include "pbg_tract.h"

namespace pbg {
extern const int kBuildKind_xpnsl = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

__device__ __forceinline__ uint64_t join(uint64_t a, uint64_t b) { return a | b; }
__device__ __forceinline__ M2 join(M2 a, M2 b) { return {a.lo | b.lo, a.hi | b.hi}; }

template <int RB>
struct XpnslWalk {
    using M = typename RowMask<RB>::T;
    static constexpr int kM = 2;
    struct Tot {
        uint64_t s0, s1;   // the sides' sums
        uint32_t c0, c1;   // the sides' agreeing pairs still at the walk's start value
    };
    M pm0, pm1, pm;
    int n0, n1, C0, C1, Pn, lane;   // Pn = C0 + C1: 0 when both sides are one sample
    int32_t *last;
    const uint16_t *uv;
    // the walk's state per side, wave-uniform: the sum of last[] and the pairs still at the start value
    int64_t sum0, sum1;
    int32_t ne0, ne1;
    bool narrow;   // a site's sum over the wave stays below 2^32 when every distance is at most V + 1: one scan

    __device__ __forceinline__ bool is_site(const M &x) const {
        const int m = (int)pc(x);
        return m >= 1 && m <= n0 + n1 - 1;
    }
    __device__ __forceinline__ void pairs(const TractLds<RB> &L) const {
        tract_pairs(L, lane, pm0, n0, 0, 0);
        tract_pairs(L, lane, pm1, n1, n0, C0);
    }
    __device__ __forceinline__ void store_m(int32_t *o, const M &x) const {
        o[0] = (int32_t)pc(x & pm0);
        o[1] = (int32_t)pc(x & pm1);
    }
    __device__ __forceinline__ void start(int V, int edge) {
        narrow = ((uint64_t)V + 1) * (uint64_t)(Pn > 0 ? Pn : 1) < (1ULL << 32);
        sum0 = (int64_t)C0 * edge;
        sum1 = (int64_t)C1 * edge;
        ne0 = C0;
        ne1 = C1;
    }

    // per side the sum of |k - last| over its agreeing pairs and those of them whose last is still
    // `edge`; a differing pair moves last to k
    __device__ __forceinline__ Tot site(const M &x, int k, int edge) {
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
        const Tot t{(uint64_t)all0 - dd0, (uint64_t)all1 - dd1, (uint32_t)ne0 - de0, (uint32_t)ne1 - de1};
        sum0 += fwd ? (int64_t)dd0 : -(int64_t)dd0;
        sum1 += fwd ? (int64_t)dd1 : -(int64_t)dd1;
        ne0 -= (int32_t)de0;
        ne1 -= (int32_t)de1;
        return t;
    }

    __device__ __forceinline__ void store_fwd(const TractOut &O, int k, const Tot &r) const {
        if (O.sl) {
            O.sl[2 * (size_t)k] = (int64_t)r.s0;
            O.sl[2 * (size_t)k + 1] = (int64_t)r.s1;
        }
        if (O.cens) {
            O.cens[2 * (size_t)k] = (int32_t)r.c0;
            O.cens[2 * (size_t)k + 1] = (int32_t)r.c1;
        }
    }
    __device__ __forceinline__ void store_bwd(const TractOut &O, int k, const Tot &r, const M &x) const {
        if (O.sl) {
            const int64_t m0 = (int64_t)pc(x & pm0), m1 = (int64_t)pc(x & pm1);
            O.sl[2 * (size_t)k] = load_fresh(O.sl + 2 * (size_t)k) + (int64_t)r.s0 - choose2(m0) - choose2(n0 - m0);
            O.sl[2 * (size_t)k + 1] = load_fresh(O.sl + 2 * (size_t)k + 1) + (int64_t)r.s1 - choose2(m1) - choose2(n1 - m1);
        }
        if (O.cens) {
            O.cens[2 * (size_t)k] = load_fresh(O.cens + 2 * (size_t)k) + (int32_t)r.c0;
            O.cens[2 * (size_t)k + 1] = load_fresh(O.cens + 2 * (size_t)k + 1) + (int32_t)r.c1;
        }
    }
};

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_xpnsl_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                           uint32_t n_win, TractArgs A) {
    using M = typename RowMask<RB>::T;
    extern __shared__ uint4 s_xpnsl[];
    const int np = P.npops, npairs = np * (np - 1) / 2, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t ch = (uint64_t)blockIdx.x * (uint64_t)A.waves + (uint64_t)wave;
    if (ch >= (uint64_t)n_win * (uint64_t)npairs) return;   // the whole wave
    const TractLds<RB> L(reinterpret_cast<unsigned char *>(s_xpnsl) + (size_t)wave * A.wave_bytes, A.pairs_max);
    const uint32_t w = (uint32_t)(ch / (uint64_t)npairs);
    int pi = 0, pj = (int)(ch - (uint64_t)w * (uint64_t)npairs);   // pair (pi, pj), pi < pj, lexicographic
    while (pj >= np - 1 - pi) {
        pj -= np - 1 - pi;
        ++pi;
    }
    pj += pi + 1;
    const int n0 = P.pop_n[pi], n1 = P.pop_n[pj], C0 = n0 * (n0 - 1) / 2, C1 = n1 * (n1 - 1) / 2;
    const M pm0 = pop_mask<M>(P, pi), pm1 = pop_mask<M>(P, pj);
    XpnslWalk<RB> pol{pm0, pm1, join(pm0, pm1), n0, n1, C0, C1, C0 + C1, lane, L.last, L.uv, 0, 0, 0, 0, false};
    tract_chain<RB>(rows, n_rows, clamp_window(A.wins[w], n_rows, A.err, lane), lane, A, ch, L, pol);
}

hipError_t launch_window_xpnsl(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win, TractArgs A,
                               hipStream_t stream) {
    const int npairs = P.npops * (P.npops - 1) / 2;
    if (n_win == 0 || npairs == 0) return hipSuccess;
    // both sides' pairs share a chain's table; the populations are disjoint and hold at most 126 samples,
    // so the largest C(n_i, 2) + C(n_j, 2) is at most C(126, 2), pbg_window_nsl's own worst case
    int pairs_max = 1;
    for (int i = 0; i < P.npops; ++i)
        for (int j = i + 1; j < P.npops; ++j) {
            const int c = (int)(choose2(P.pop_n[i]) + choose2(P.pop_n[j]));
            pairs_max = c > pairs_max ? c : pairs_max;
        }
    TractPlan plan;
    if (!tract_plan(rb, pairs_max, (uint64_t)n_win * (uint64_t)npairs, A, plan)) return hipErrorInvalidValue;
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_xpnsl_kernel<decltype(RB)::value>, plan.grid, plan.block, plan.lds, stream, P, rows, n_rows,
                           n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
