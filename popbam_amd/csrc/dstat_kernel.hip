// dstat_kernel.hip -- Patterson's D (ABBA-BABA), f_d and f_dM on gfx950, per window and population
// triple (pbg_window_dstat; no reference counterpart, DESIGN.md "D statistics").
//
// For a segregating row with sample bits t and a triple (P1, P2, P3) of sizes n1, n2, n3:
// a = popcount(t & mask_P1), b and c alike, all three flipped (n - count) when the outgroup carries
// the derived allele.  Six int64 sums per (window, triple) -- ABBA, BABA and the four donor-split
// denominators of f_d and f_dM -- and three doubles formed from them (include/popbam_gpu.h has the
// definition).
//
// One workgroup per window.  The rows are streamed as in jsfs_kernel.hip: every wave takes 16-byte
// row words, the next ones loaded ahead, packs the segregating rows it finds into a queue of its own
// (wave prefix sum) and parks every queued row's per-population counts as bytes, flip included.  The
// triple work reads three bytes per (row, triple); its lane mapping follows the list's length:
//   up to kDstatLaneTriples triples: with G the power of two >= n_triples, lane l owns triple
//     l & (G - 1) for the whole window and takes rows l / G, l / G + 64 / G, ... of every batch; its
//     six sums stay in registers, and after the last row a butterfly over the lanes of one triple and
//     one integer LDS add per wave combine them.  Segregating rows are sparse (a dozen per wave
//     iteration at 10 kb windows), so a lane per triple alone would idle most of the wave.
//   longer lists: a lane per triple of the group over the batch's rows, the batch's six partial sums
//     added to the group's LDS sums with integer atomics (no two lanes of a wave share an address).
// Integer adds are order-free: two runs give the same bytes.  Lists longer than kDstatLdsTriples go
// in groups, the rows streamed once per group.  After a group's rows one lane per triple writes the
// sums and forms D, f_d and f_dM.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_dstat = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

// a queued row: the sample bits in the narrowest word that holds them
template <int RB>
struct DstatQ {
    using T = uint32_t;
    __device__ __forceinline__ static T put(uint64_t t) { return (uint32_t)t; }
    __device__ __forceinline__ static uint64_t get(T q) { return q; }
};
template <>
struct DstatQ<8> {
    using T = uint64_t;
    __device__ __forceinline__ static T put(uint64_t t) { return t; }
    __device__ __forceinline__ static uint64_t get(T q) { return q; }
};
template <>
struct DstatQ<16> {
    using T = M2;
    __device__ __forceinline__ static T put(M2 t) { return t; }
    __device__ __forceinline__ static M2 get(T q) { return q; }
};

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the six sums of one triple (named members: they stay in registers)
struct Sums6 {
    long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0;
    template <class F>
    __device__ __forceinline__ void each(F f) {   // f(index, sum)
        f(0, s0), f(1, s1), f(2, s2), f(3, s3), f(4, s4), f(5, s5);
    }
};

// one site's six terms (include/popbam_gpu.h); every product stays below 2^21
__device__ __forceinline__ void dstat_terms(int a, int b, int c, int n1, int n2, int n3, Sums6 &s) {
    s.s0 += (n1 - a) * b * c;
    s.s1 += a * (n2 - b) * c;
    const bool d2 = b * n3 >= c * n2, d1 = a * n3 >= c * n1;
    s.s2 += d2 ? b * (b * n1 - a * n2) : 0;
    s.s3 += d2 ? 0 : c * (c * n1 - a * n3);
    s.s4 += d1 ? a * (a * n2 - b * n1) : 0;
    s.s5 += d1 ? 0 : c * (c * n2 - b * n3);
}

__device__ __forceinline__ double dstat_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// the unit is built with -ffp-contract=off: every conversion, division and sum is its own IEEE operation
__device__ __forceinline__ void dstat_ratios(const Sums6 &s, int n1, int n2, int n3, double &d, double &fd, double &fdm) {
    const long long l1 = n1, l2 = n2, l3 = n3;
    const double diff = (double)(s.s0 - s.s1);
    const double num = diff / (double)(l1 * l2 * l3);
    const double den = (double)s.s2 / (double)(l1 * l2 * l2) + (double)s.s3 / (double)(l1 * l3 * l3);
    const double den2 = (double)s.s4 / (double)(l2 * l1 * l1) + (double)s.s5 / (double)(l2 * l3 * l3);
    d = s.s0 + s.s1 == 0 ? dstat_nan() : diff / (double)(s.s0 + s.s1);
    fd = den == 0.0 ? dstat_nan() : num / den;
    const double dm = s.s0 >= s.s1 ? den : den2;
    fdm = dm == 0.0 ? dstat_nan() : num / dm;
}

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_dstat_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                           uint32_t n_win, DstatArgs A) {
    using M = typename RowMask<RB>::T;
    using Q = DstatQ<RB>;
    constexpr int R = 16 / RB;
    constexpr int QCAP = 64 * R;   // the rows one wave decodes per iteration
    extern __shared__ __align__(16) unsigned char sm[];
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(sm);   // [6][ntg] of the group
    __shared__ typename Q::T s_q[4][QCAP];
    __shared__ uint8_t s_cnt[4][kDstatCntBytes];
    __shared__ uint64_t s_pm[PBG_MAX_POPS], s_pmh[PBG_MAX_POPS];
    __shared__ int32_t s_pn[PBG_MAX_POPS];
    __shared__ uint32_t s_tw[kDstatLdsTriples];   // the group's triple words
    const int np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t w = blockIdx.x;
    if (w >= n_win) return;
    if (tid < np) {
        s_pm[tid] = P.pop_mask[tid];
        s_pmh[tid] = P.pop_mask_hi[tid];
        s_pn[tid] = P.pop_n[tid];
    }
    auto pmask = [&](int i) -> M {
        if constexpr (RB == 16) return M2{s_pm[i], s_pmh[i]};
        else return s_pm[i];
    };
    int64_t wb = A.wins[w].beg, we = A.wins[w].end;
    if (we <= wb) {
        wb = we = 0;   // an empty window, whatever its coordinates
    } else if (wb < 0 || we > (int64_t)n_rows) {
        // a window outside the rows is reported (pbg_check -> PBG_E_RANGE) and never read
        if (tid == 0) atomicOr(A.err, 4);
        wb = we = 0;
    }
    const int64_t c0 = wb / R, c1 = (we + R - 1) / R;
    const int batch = kDstatCntBytes / np;   // rows whose counts are staged together (>= 16)
    const int outidx = A.outidx;
    const int nt = A.n_triples;
    // short lists: lane -> (triple my, first row slot) for the whole window
    const bool by_lane = nt <= kDstatLaneTriples;   // kernel-uniform
    int G = 1;
    while (G < nt) G <<= 1;
    const int my = lane & (G - 1), slot = by_lane ? lane / G : 0, step = by_lane ? 64 / G : 1;

    for (int t0 = 0; t0 < nt; t0 += kDstatLdsTriples) {
        const int ntg = nt - t0 < kDstatLdsTriples ? nt - t0 : kDstatLdsTriples;
        __syncthreads();   // the masks; the previous group's readers
        for (int k = tid; k < ntg * 6; k += 256) s_acc[k] = 0;
        for (int k = tid; k < ntg; k += 256) s_tw[k] = A.triples[t0 + k];
        __syncthreads();
        const bool have = by_lane && my < ntg;
        int i1 = 0, i2 = 0, i3 = 0, n1 = 0, n2 = 0, n3 = 0;
        if (have) {
            const uint32_t tw = s_tw[my];
            i1 = (int)(tw & 63u), i2 = (int)(tw >> 6) & 63, i3 = (int)(tw >> 12) & 63;
            n1 = s_pn[i1], n2 = s_pn[i2], n3 = s_pn[i3];
        }
        Sums6 acc;

        // ---- the window's rows: every wave takes 64 words at a time, the next ones loaded ahead
        uint4 nxt = make_uint4(0, 0, 0, 0);
        if (c0 + wave * 64 + lane < c1) nxt = load_row_word<RB>(rows, n_rows, c0 + wave * 64 + lane);
        for (int64_t cb = c0 + wave * 64; cb < c1; cb += 256) {   // wave-uniform
            const int64_t c = cb + lane;
            const uint4 q = nxt;
            nxt = c + 256 < c1 ? load_row_word<RB>(rows, n_rows, c + 256) : make_uint4(0, 0, 0, 0);
            M t[R];
            uint32_t vm = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t ri = c * R + r;
                bool cnt, sg;
                row_in_word<RB>(q, r, t[r], cnt, sg);
                vm |= (c < c1 && ri >= wb && ri < we && sg) ? (1u << r) : 0u;
            }
            const uint32_t ls = (uint32_t)__popc(vm);
            const uint32_t incl = wave_incl_scan_s(ls);
            uint32_t j = incl - ls;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if ((vm >> r) & 1u) s_q[wave][j++] = Q::put(t[r]);
            const int nq = __builtin_amdgcn_readlane((int)incl, 63);
            if (nq == 0) continue;
            wave_sync();
            for (int b0 = 0; b0 < nq; b0 += batch) {
                const int nb = nq - b0 < batch ? nq - b0 : batch;
                // (row, population): each count once, flipped when the outgroup is derived
                for (int k = lane; k < nb * np; k += 64) {
                    const int row = k / np, i = k - row * np;
                    const M tt = Q::get(s_q[wave][b0 + row]);
                    int f = (int)pc(tt & pmask(i));
                    if (outidx >= 0 && bit(tt, outidx)) f = s_pn[i] - f;
                    s_cnt[wave][k] = (uint8_t)f;
                }
                wave_sync();
                if (by_lane) {
                    if (have)
                        for (int row = slot; row < nb; row += step) {
                            const uint8_t *cn = &s_cnt[wave][row * np];
                            dstat_terms(cn[i1], cn[i2], cn[i3], n1, n2, n3, acc);
                        }
                } else {
                    for (int tr = lane; tr < ntg; tr += 64) {
                        const uint32_t tw = s_tw[tr];
                        const int j1 = (int)(tw & 63u), j2 = (int)(tw >> 6) & 63, j3 = (int)(tw >> 12) & 63;
                        const int m1 = s_pn[j1], m2 = s_pn[j2], m3 = s_pn[j3];
                        Sums6 v;
                        for (int row = 0; row < nb; ++row) {
                            const uint8_t *cn = &s_cnt[wave][row * np];
                            dstat_terms(cn[j1], cn[j2], cn[j3], m1, m2, m3, v);
                        }
                        v.each([&](int x, long long sx) { atomicAdd(&s_acc[x * ntg + tr], (unsigned long long)sx); });
                    }
                }
                wave_sync();   // the next batch's counts, the next iteration's queue
            }
        }
        if (by_lane) {
            // the lanes of one triple are G apart: an integer butterfly, then one add per wave
            acc.each([&](int x, long long v) {
                for (int dd = 32; dd >= G; dd >>= 1) v += __shfl_xor(v, dd, 64);
                if (lane < ntg) atomicAdd(&s_acc[x * ntg + lane], (unsigned long long)v);
            });
        }
        __syncthreads();

        // ---- the group's results: a lane per triple
        for (int tr = tid; tr < ntg; tr += 256) {
            const uint32_t tw = s_tw[tr];
            const int m1 = s_pn[tw & 63u], m2 = s_pn[(tw >> 6) & 63u], m3 = s_pn[(tw >> 12) & 63u];
            Sums6 s;
            s.s0 = (long long)s_acc[tr], s.s1 = (long long)s_acc[ntg + tr], s.s2 = (long long)s_acc[2 * ntg + tr];
            s.s3 = (long long)s_acc[3 * ntg + tr], s.s4 = (long long)s_acc[4 * ntg + tr], s.s5 = (long long)s_acc[5 * ntg + tr];
            const size_t o = (size_t)w * (size_t)nt + (size_t)(t0 + tr);
            if (A.sums) s.each([&](int x, long long sx) { A.sums[o * 6 + x] = sx; });
            if (A.d || A.fd || A.fdm) {   // kernel-uniform
                double d, fd, fdm;
                dstat_ratios(s, m1, m2, m3, d, fd, fdm);
                if (A.d) A.d[o] = d;
                if (A.fd) A.fd[o] = fd;
                if (A.fdm) A.fdm[o] = fdm;
            }
        }
    }
}

template __global__ void window_dstat_kernel<2>(DevParams, const void *, uint32_t, uint32_t, DstatArgs);
template __global__ void window_dstat_kernel<4>(DevParams, const void *, uint32_t, uint32_t, DstatArgs);
template __global__ void window_dstat_kernel<8>(DevParams, const void *, uint32_t, uint32_t, DstatArgs);
template __global__ void window_dstat_kernel<16>(DevParams, const void *, uint32_t, uint32_t, DstatArgs);

hipError_t launch_window_dstat(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                               const DstatArgs &A, hipStream_t stream) {
    if (n_win == 0 || A.n_triples <= 0) return hipSuccess;
    const dim3 g(n_win), b(256);
    const size_t lds = (size_t)(A.n_triples < kDstatLdsTriples ? A.n_triples : kDstatLdsTriples) * 48;
    switch (rb) {
        case 2: hipLaunchKernelGGL(window_dstat_kernel<2>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
        case 4: hipLaunchKernelGGL(window_dstat_kernel<4>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
        case 8: hipLaunchKernelGGL(window_dstat_kernel<8>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
        default: hipLaunchKernelGGL(window_dstat_kernel<16>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
    }
    return hipGetLastError();
}

}  // namespace pbg
