// hfs_kernel.hip -- the haplotype frequency spectrum and Garud's H1, H12, H123, H2/H1 on gfx950, per
// window and population (pbg_window_hfs; no reference counterpart, DESIGN.md "Haplotype frequency
// spectrum").
//
// Two samples of a population are in one class iff their bits agree in every segregating row of the
// window.  No hashing: sample s gets a difference mask D_s = OR over the rows t of (bit s of t ? ~t : t),
// whose bit u says that s and u differ somewhere.  The lowest set bit of ~D_s inside the population's
// mask is the class's lowest member (equality is an equivalence), its rank inside the mask the label.
//
// One workgroup per window.  The window's segregating rows come through the row stream
// (pbg_rows.h), a wave's queue at a time.  With G the power of two >= n_samples (at most 64), lane l
// owns sample l & (G - 1) for the whole window -- above 64 samples also sample l + 64 -- and takes queued rows
// l / G, l / G + 64 / G, ...; its masks stay in registers.  After the last row an OR butterfly over
// the lanes of one sample and one integer LDS OR per sample and wave merge them.  Then the workgroup
// labels the samples, counts the class sizes in an LDS histogram, sorts each population's sizes by
// rank (slot j counts the sizes that go before its own) and forms the sums and the five doubles.
// Integer ORs and adds only: two runs give the same bytes.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_hfs = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

// a difference mask has the type of a queued row (QueuedRow, pbg_rows.h)
template <int RB>
struct HfsQ : QueuedRow<RB> {
    using T = typename QueuedRow<RB>::T;
    __device__ __forceinline__ static T zero() { return 0u; }
    // D |= (bit s of t ? ~t : t)
    __device__ __forceinline__ static void differ(T &d, T t, int s) { d |= t ^ (0u - ((t >> s) & 1u)); }
    __device__ __forceinline__ static void merge(T &d, int dd) { d |= (uint32_t)__shfl_xor((int)d, dd, 64); }
    __device__ __forceinline__ static uint64_t lo(T d) { return d; }
    __device__ __forceinline__ static uint64_t hi(T) { return 0; }
};
template <>
struct HfsQ<8> : QueuedRow<8> {
    __device__ __forceinline__ static T zero() { return 0ull; }
    __device__ __forceinline__ static void differ(T &d, T t, int s) { d |= t ^ (0ull - ((t >> s) & 1ull)); }
    __device__ __forceinline__ static void merge(T &d, int dd) { d |= (uint64_t)__shfl_xor((unsigned long long)d, dd, 64); }
    __device__ __forceinline__ static uint64_t lo(T d) { return d; }
    __device__ __forceinline__ static uint64_t hi(T) { return 0; }
};
template <>
struct HfsQ<16> : QueuedRow<16> {
    __device__ __forceinline__ static T zero() { return M2{0ull, 0ull}; }
    __device__ __forceinline__ static void differ(T &d, T t, int s) {
        const uint64_t m = 0ull - (uint64_t)bit(t, s);
        d.lo |= t.lo ^ m;
        d.hi |= t.hi ^ m;
    }
    __device__ __forceinline__ static void merge(T &d, int dd) {
        d.lo |= (uint64_t)__shfl_xor((unsigned long long)d.lo, dd, 64);
        d.hi |= (uint64_t)__shfl_xor((unsigned long long)d.hi, dd, 64);
    }
    __device__ __forceinline__ static uint64_t lo(T d) { return d.lo; }
    __device__ __forceinline__ static uint64_t hi(T d) { return d.hi; }
};

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_hfs_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                         uint32_t n_win, HfsArgs A) {
    using Q = HfsQ<RB>;
    using D = typename Q::T;
    __shared__ D s_q[4][64 * (16 / RB)];
    __shared__ unsigned long long s_dlo[kHfsSlots], s_dhi[kHfsSlots];   // the samples' difference masks
    __shared__ int32_t s_hist[kHfsSlots], s_sorted[kHfsSlots];          // class sizes, by population (pop_start)
    __shared__ PopLds s_pop;
    __shared__ int16_t s_pst[PBG_MAX_POPS + 1];
    __shared__ int8_t s_spop[kHfsSlots];    // population of a sample
    __shared__ int8_t s_slpop[kHfsSlots];   // population of a histogram slot
    const int n = P.n, np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t w = blockIdx.x;
    if (w >= n_win) return;
    s_pop.stage(P, tid);
    if (tid <= np) s_pst[tid] = P.pop_start[tid];
    if (tid < kHfsSlots) {
        s_dlo[tid] = 0;
        s_dhi[tid] = 0;
        s_hist[tid] = 0;
        s_spop[tid] = tid < n ? P.sample_pop[tid] : (int8_t)-1;
        s_slpop[tid] = tid < P.pop_start[np] ? P.sample_pop[P.pop_member[tid]] : (int8_t)-1;
    }
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, tid);
    const bool empty = win.empty;
    // lane -> (sample sa, and sb = sa + 64 above 64 samples; first row slot) for the whole window
    int G = 1;
    while (G < n && G < 64) G <<= 1;
    const int sa = lane & (G - 1), sb = sa + 64, slot = lane / G, step = 64 / G;
    D da = Q::zero(), db = Q::zero();
    __syncthreads();   // the zeroed masks

    // ---- the window's rows (pbg_rows.h): two words loaded ahead (a window is one workgroup, so a
    // launch of few, long windows has little else in flight to hide the latency)
    stream_window_rows<RB, 2>(rows, n_rows, win, wave, lane, s_q[wave], [&](int nq) {
        for (int row = slot; row < nq; row += step) {
            const D tt = s_q[wave][row];
            Q::differ(da, tt, sa);
            if constexpr (RB == 16) Q::differ(db, tt, sb & 127);   // counts only when sb < n
        }
    });
    // the lanes of one sample are G apart: an OR butterfly, then one LDS OR per sample and wave
    for (int dd = 32; dd >= G; dd >>= 1) {
        Q::merge(da, dd);
        if constexpr (RB == 16) Q::merge(db, dd);
    }
    if (lane < G && sa < n) {
        if (Q::lo(da)) atomicOr(&s_dlo[sa], (unsigned long long)Q::lo(da));
        if constexpr (RB == 16) {
            if (Q::hi(da)) atomicOr(&s_dhi[sa], (unsigned long long)Q::hi(da));
            if (sb < n) {
                if (Q::lo(db)) atomicOr(&s_dlo[sb], (unsigned long long)Q::lo(db));
                if (Q::hi(db)) atomicOr(&s_dhi[sb], (unsigned long long)Q::hi(db));
            }
        }
    }
    __syncthreads();

    // ---- a thread per sample: its class is the rank of the lowest member that equals it
    if (tid < n) {
        const int i = s_spop[tid];
        int label = 255;
        if (i >= 0 && !empty) {
            // bit tid of the candidates is always set (a sample equals itself), so a lower word decides first
            const uint64_t lo = ~s_dlo[tid] & s_pop.pm[i], hi = ~s_dhi[tid] & s_pop.pmh[i];
            if (lo) {
                const int f = __builtin_ctzll(lo);
                label = (int)pc(s_pop.pm[i] & ((1ull << f) - 1ull));
            } else {
                const int f = __builtin_ctzll(hi | (1ull << 63));
                label = (int)(pc(s_pop.pm[i]) + pc(s_pop.pmh[i] & ((1ull << f) - 1ull)));
            }
            atomicAdd(&s_hist[s_pst[i] + label], 1);   // label < the population's members
        }
        if (A.cls) A.cls[(size_t)w * (size_t)n + (size_t)tid] = (uint8_t)label;
    }
    __syncthreads();

    // ---- a thread per histogram slot: descending order by rank (ties: the lower slot first)
    if (tid < kHfsSlots) {
        const int i = s_slpop[tid];
        if (i >= 0) {
            const int a0 = s_pst[i], a1 = s_pst[i + 1], cj = s_hist[tid];
            int rank = 0;
            for (int k = a0; k < a1; ++k) {
                const int ck = s_hist[k];
                rank += (ck > cj || (ck == cj && k < tid)) ? 1 : 0;
            }
            s_sorted[a0 + rank] = cj;
        }
    }
    __syncthreads();

    // ---- the outputs
    const int stride = P.pop_nmax;
    if (A.counts)
        for (int k = tid; k < np * stride; k += 256) {
            const int i = k / stride, r = k - i * stride;
            const int a0 = s_pst[i], cnt = s_pst[i + 1] - a0;
            A.counts[((size_t)w * (size_t)np) * (size_t)stride + (size_t)k] = r < cnt ? s_sorted[a0 + r] : 0;
        }
    for (int i = tid; i < np; i += 256) {
        const int a0 = s_pst[i], cnt = s_pst[i + 1] - a0;
        long long qq = 0;
        int kk = 0;
        for (int r = 0; r < cnt; ++r) {
            const long long cr = s_sorted[a0 + r];
            qq += cr * cr;
            kk += cr > 0 ? 1 : 0;
        }
        const long long x1 = cnt > 0 ? s_sorted[a0] : 0, x2 = cnt > 1 ? s_sorted[a0 + 1] : 0, x3 = cnt > 2 ? s_sorted[a0 + 2] : 0;
        const size_t o = (size_t)w * (size_t)np + (size_t)i;
        if (A.k) A.k[o] = kk;
        if (A.sums) {
            A.sums[o * 4 + 0] = qq;
            A.sums[o * 4 + 1] = x1;
            A.sums[o * 4 + 2] = x2;
            A.sums[o * 4 + 3] = x3;
        }
        if (A.h) {
            // the unit is built with -ffp-contract=off: every conversion and division is its own IEEE operation
            const long long ni = s_pop.pn[i], n2 = ni * ni;
            double h1 = quiet_nan(), h12 = h1, h123 = h1, h2h1 = h1, hd = h1;
            if (!empty) {
                h1 = (double)qq / (double)n2;
                h12 = (double)(qq + 2 * x1 * x2) / (double)n2;
                h123 = (double)(qq + 2 * (x1 * x2 + x1 * x3 + x2 * x3)) / (double)n2;
                h2h1 = (double)(qq - x1 * x1) / (double)qq;
                if (ni >= 2) hd = (double)(n2 - qq) / (double)(ni * (ni - 1));
            }
            A.h[o * 5 + 0] = h1;
            A.h[o * 5 + 1] = h12;
            A.h[o * 5 + 2] = h123;
            A.h[o * 5 + 3] = h2h1;
            A.h[o * 5 + 4] = hd;
        }
    }
}

hipError_t launch_window_hfs(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                             const HfsArgs &A, hipStream_t stream) {
    if (n_win == 0) return hipSuccess;
    const dim3 g(n_win), b(256);
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_hfs_kernel<decltype(RB)::value>, g, b, 0, stream, P, rows, n_rows, n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
