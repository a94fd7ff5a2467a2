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
// The walk itself -- the passes, the LDS, the launch plan -- is pbg_tract.h's; this file is the chain
// decode and the statistic: the population's pairs in one table, the class sums of a site, P_c.
#include "pbg_common.h"
#include "pbg_rows.h"
#include "pbg_tract.h"

namespace pbg {
extern const int kBuildKind_nsl = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

template <int RB>
struct NslWalk {
    using M = typename RowMask<RB>::T;
    static constexpr int kM = 1;
    struct Tot {
        uint64_t s0, s1;   // the classes' sums
        uint32_t c;        // the agreeing pairs still at the walk's start value
    };
    M pm;
    int nn, Pn, lane;   // Pn >= 1: a variable site needs two samples
    int32_t *last;
    const uint16_t *uv;

    __device__ __forceinline__ bool is_site(const M &x) const {
        const int m = (int)pc(x);
        return m >= 1 && m <= nn - 1;
    }
    __device__ __forceinline__ void pairs(const TractLds<RB> &L) const { tract_pairs(L, lane, pm, nn, 0, 0); }
    __device__ __forceinline__ void store_m(int32_t *o, const M &x) const { *o = (int32_t)pc(x); }
    __device__ __forceinline__ void start(int, int) {}

    // the lanes' pairs against column x; an agreeing pair adds |k - last| to its class and counts as
    // censored while last is still `edge`, a differing pair moves last to k
    __device__ __forceinline__ Tot site(const M &x, int k, int edge) const {
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
        return {wave_sum38(a0), wave_sum38(a1), wave_sum32(ce)};
    }

    __device__ __forceinline__ void store_fwd(const TractOut &O, int k, const Tot &r) const {
        if (O.sl) {
            O.sl[2 * (size_t)k] = (int64_t)r.s0;
            O.sl[2 * (size_t)k + 1] = (int64_t)r.s1;
        }
        if (O.cens) O.cens[2 * (size_t)k] = (int32_t)r.c;
    }
    __device__ __forceinline__ void store_bwd(const TractOut &O, int k, const Tot &r, const M &x) const {
        if (O.sl) {
            const int64_t m = (int64_t)pc(x);
            O.sl[2 * (size_t)k] = load_fresh(O.sl + 2 * (size_t)k) + (int64_t)r.s0 - choose2(nn - m);
            O.sl[2 * (size_t)k + 1] = load_fresh(O.sl + 2 * (size_t)k + 1) + (int64_t)r.s1 - choose2(m);
        }
        if (O.cens) O.cens[2 * (size_t)k + 1] = (int32_t)r.c;
    }
};

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_nsl_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                         uint32_t n_win, TractArgs A) {
    using M = typename RowMask<RB>::T;
    extern __shared__ uint4 s_nsl[];
    const int np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t ch = (uint64_t)blockIdx.x * (uint64_t)A.waves + (uint64_t)wave;
    if (ch >= (uint64_t)n_win * (uint64_t)np) return;   // the whole wave
    const TractLds<RB> L(reinterpret_cast<unsigned char *>(s_nsl) + (size_t)wave * A.wave_bytes, A.pairs_max);
    const uint32_t w = (uint32_t)(ch / (uint64_t)np);
    const int i = (int)(ch - (uint64_t)w * (uint64_t)np), nn = P.pop_n[i];
    NslWalk<RB> pol{pop_mask<M>(P, i), nn, nn * (nn - 1) / 2, lane, L.last, L.uv};
    tract_chain<RB>(rows, n_rows, clamp_window(A.wins[w], n_rows, A.err, lane), lane, A, ch, L, pol);
}

hipError_t launch_window_nsl(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win, TractArgs A,
                             hipStream_t stream) {
    if (n_win == 0) return hipSuccess;
    int nmax = 2;
    for (int i = 0; i < P.npops; ++i) nmax = P.pop_n[i] > nmax ? P.pop_n[i] : nmax;
    TractPlan plan;
    if (!tract_plan(rb, nmax * (nmax - 1) / 2, (uint64_t)n_win * (uint64_t)P.npops, A, plan)) return hipErrorInvalidValue;
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_nsl_kernel<decltype(RB)::value>, plan.grid, plan.block, plan.lds, stream, P, rows, n_rows,
                           n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
