// dstat_kernel.hip -- Patterson's D (ABBA-BABA), f_d and f_dM on gfx950, per window and population
// triple (pbg_window_dstat; no reference counterpart, DESIGN.md "D statistics").
//
// For a segregating row with sample bits t and a triple (P1, P2, P3) of sizes n1, n2, n3:
// a = popcount(t & mask_P1), b and c alike, all three flipped (n - count) when the outgroup carries
// the derived allele.  Six int64 sums per (window, triple) -- ABBA, BABA and the four donor-split
// denominators of f_d and f_dM -- and three doubles formed from them (include/popbam_gpu.h has the
// definition).
//
// One workgroup per window.  The window's segregating rows come through the row stream and every
// queued row's per-population counts, flip included, through the count batches (both in
// pbg_rows.h).  The triple work reads three bytes per (row, triple) of a batch; its lane mapping
// follows the list's length:
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

// the unit is built with -ffp-contract=off: every conversion, division and sum is its own IEEE operation
__device__ __forceinline__ void dstat_ratios(const Sums6 &s, int n1, int n2, int n3, double &d, double &fd, double &fdm) {
    const long long l1 = n1, l2 = n2, l3 = n3;
    const double diff = (double)(s.s0 - s.s1);
    const double num = diff / (double)(l1 * l2 * l3);
    const double den = (double)s.s2 / (double)(l1 * l2 * l2) + (double)s.s3 / (double)(l1 * l3 * l3);
    const double den2 = (double)s.s4 / (double)(l2 * l1 * l1) + (double)s.s5 / (double)(l2 * l3 * l3);
    d = s.s0 + s.s1 == 0 ? quiet_nan() : diff / (double)(s.s0 + s.s1);
    fd = den == 0.0 ? quiet_nan() : num / den;
    const double dm = s.s0 >= s.s1 ? den : den2;
    fdm = dm == 0.0 ? quiet_nan() : num / dm;
}

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_dstat_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                           uint32_t n_win, DstatArgs A) {
    using Q = QueuedRow<RB>;
    extern __shared__ __align__(16) unsigned char sm[];
    unsigned long long *s_acc = reinterpret_cast<unsigned long long *>(sm);   // [6][ntg] of the group
    __shared__ typename Q::T s_q[4][64 * (16 / RB)];
    __shared__ uint8_t s_cnt[4][kCntBytes];
    __shared__ PopLds s_pop;
    __shared__ uint32_t s_tw[kDstatLdsTriples];   // the group's triple words
    const int np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t w = blockIdx.x;
    if (w >= n_win) return;
    s_pop.stage(P, tid);
    const int32_t *s_pn = s_pop.pn;
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, tid);
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

        // ---- the window's rows (pbg_rows.h): one word loaded ahead
        stream_window_rows<RB, 1>(rows, n_rows, win, wave, lane, s_q[wave], [&](int nq) {
            count_batches<RB>(s_q[wave], nq, s_pop, np, A.outidx, lane, s_cnt[wave], [&](int nb) {
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
            });
        });
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

hipError_t launch_window_dstat(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                               const DstatArgs &A, hipStream_t stream) {
    if (n_win == 0 || A.n_triples <= 0) return hipSuccess;
    const dim3 g(n_win), b(256);
    const size_t lds = (size_t)(A.n_triples < kDstatLdsTriples ? A.n_triples : kDstatLdsTriples) * 48;
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_dstat_kernel<decltype(RB)::value>, g, b, lds, stream, P, rows, n_rows, n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
