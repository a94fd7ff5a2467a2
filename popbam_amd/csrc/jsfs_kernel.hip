// jsfs_kernel.hip -- joint site-frequency spectrum, pairwise-difference counts and Fst on gfx950,
// per window and population pair (pbg_window_jsfs; no reference counterpart, DESIGN.md "Joint SFS").
//
// For a segregating row with sample bits t and populations i < j: a = popcount(t & mask_i),
// b = popcount(t & mask_j), both flipped (n - count) when the outgroup carries the derived allele.
// J_p[a][b] counts the window's segregating rows; SW_i = sum a(n_i - a), SW_j = sum b(n_j - b),
// SB = sum a(n_j - b) + b(n_i - a) and Hudson's Fst follow from the finished histogram
// (include/popbam_gpu.h has the definition).
//
// One workgroup per window, the histogram in LDS.  The pairs are taken in groups of consecutive
// pairs whose cells fit kJsfsLdsCells (the host plans them; most contexts have one group); per group
// every wave streams 16-byte row words of the window, packs the segregating rows it finds into a
// queue of its own (wave prefix sum), then works through flat item lists so that no lane idles
// behind another lane's row: (row, population) items form each count once and park it as a byte,
// (row, pair) items read two bytes and bump one cell with an integer LDS atomic.  The counts are
// staged for kJsfsCntBytes / n_pops rows at a time.  Integer atomics are order-free: two runs give
// the same bytes.  No list of sites outlives an iteration, so there is no capacity and no workspace.
// After a group's rows: the cells are copied out, the three sums are int64 sums of cell * weight (a
// lane per pair of up to 64 cells, a wave per larger pair with an integer butterfly) and one lane
// per pair forms Fst.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_jsfs = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

// a queued row: the sample bits in the narrowest word that holds them
template <int RB>
struct JsfsQ {
    using T = uint32_t;
    __device__ __forceinline__ static T put(uint64_t t) { return (uint32_t)t; }
    __device__ __forceinline__ static uint64_t get(T q) { return q; }
};
template <>
struct JsfsQ<8> {
    using T = uint64_t;
    __device__ __forceinline__ static T put(uint64_t t) { return t; }
    __device__ __forceinline__ static uint64_t get(T q) { return q; }
};
template <>
struct JsfsQ<16> {
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

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Hudson's estimator as a ratio of sums (include/popbam_gpu.h); the unit is built with
// -ffp-contract=off, so the product and the sums stay separate IEEE operations
__device__ __forceinline__ double jsfs_fst(long long swi, long long swj, long long sb, int ni, int nj) {
    if (ni < 2 || nj < 2 || sb == 0) return __longlong_as_double(0x7FF8000000000000LL);
    const double pw_i = (double)swi / (double)(ni * (ni - 1) / 2);
    const double pw_j = (double)swj / (double)(nj * (nj - 1) / 2);
    const double pb = (double)sb / (double)(ni * nj);
    return 1.0 - (0.5 * (pw_i + pw_j)) / pb;
}

// cells [k0, k0 + stride, ...) of one pair's histogram: the three weighted sums
__device__ __forceinline__ void jsfs_sums(const int32_t *h, int cells, int ni, int nj, int k0, int stride, long long &swi,
                                          long long &swj, long long &sb) {
    const int nj1 = nj + 1;
    for (int k = k0; k < cells; k += stride) {
        const int a = k / nj1, b = k - a * nj1;
        const long long c = h[k];
        swi += c * (long long)(a * (ni - a));
        swj += c * (long long)(b * (nj - b));
        sb += c * (long long)(a * (nj - b) + b * (ni - a));
    }
}

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_jsfs_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                          uint32_t n_win, JsfsArgs A) {
    using M = typename RowMask<RB>::T;
    using Q = JsfsQ<RB>;
    constexpr int R = 16 / RB;
    constexpr int QCAP = 64 * R;   // the rows one wave decodes per iteration
    extern __shared__ __align__(16) unsigned char sm[];
    int32_t *s_cells = reinterpret_cast<int32_t *>(sm);
    __shared__ typename Q::T s_q[4][QCAP];
    __shared__ uint8_t s_cnt[4][kJsfsCntBytes];
    __shared__ uint64_t s_pm[PBG_MAX_POPS], s_pmh[PBG_MAX_POPS];
    __shared__ int32_t s_pn[PBG_MAX_POPS];
    __shared__ uint32_t s_pw[PBG_MAX_POPS * (PBG_MAX_POPS - 1) / 2];   // the group's pair words
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
    const int batch = kJsfsCntBytes / np;   // rows whose counts are staged together (>= 16)
    const int outidx = A.outidx;

    for (int g = 0; g < A.n_groups; ++g) {
        const int p0 = A.groups[g], p1 = A.groups[g + 1], npg = p1 - p0;
        const int base = (int)(A.pairs[p0] & 0x7FFFu);
        const int ncell = (p1 < A.n_pairs ? (int)(A.pairs[p1] & 0x7FFFu) : A.n_cells) - base;
        __syncthreads();   // the masks; the previous group's readers
        for (int k = tid; k < ncell; k += 256) s_cells[k] = 0;
        for (int k = tid; k < npg; k += 256) s_pw[k] = A.pairs[p0 + k];   // off the row loop's dependent chain
        __syncthreads();

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
                // (row, pair of this group): one cell each
                for (int k = lane; k < nb * npg; k += 64) {
                    const int row = k / npg, pr = k - row * npg;
                    const uint32_t pw = s_pw[pr];
                    const int i = (int)(pw >> 15) & 63, jj = (int)(pw >> 21) & 63;
                    const int a = s_cnt[wave][row * np + i], b = s_cnt[wave][row * np + jj];
                    const int idx = (int)(pw & 0x7FFFu) - base + a * (s_pn[jj] + 1) + b;
                    if ((uint32_t)idx < (uint32_t)ncell) atomicAdd(&s_cells[idx], 1);
                }
                wave_sync();   // the next batch's counts, the next iteration's queue
            }
        }
        __syncthreads();

        // ---- the group's results
        if (A.cells)
            for (int k = tid; k < ncell; k += 256) A.cells[(size_t)w * (size_t)A.n_cells + (size_t)(base + k)] = s_cells[k];
        auto emit = [&](int p, long long swi, long long swj, long long sb, int ni, int nj) {
            const size_t o = (size_t)w * (size_t)A.n_pairs + (size_t)p;
            if (A.diffs) {
                A.diffs[o * 3] = swi;
                A.diffs[o * 3 + 1] = swj;
                A.diffs[o * 3 + 2] = sb;
            }
            if (A.fst) A.fst[o] = jsfs_fst(swi, swj, sb, ni, nj);
        };
        for (int p = p0 + tid; p < p1; p += 256) {   // pairs of up to 64 cells: a lane each
            const uint32_t pw = s_pw[p - p0];
            const int ni = s_pn[(pw >> 15) & 63], nj = s_pn[(pw >> 21) & 63], cells = (ni + 1) * (nj + 1);
            if (cells > 64) continue;
            long long swi = 0, swj = 0, sb = 0;
            jsfs_sums(s_cells + ((int)(pw & 0x7FFFu) - base), cells, ni, nj, 0, 1, swi, swj, sb);
            emit(p, swi, swj, sb, ni, nj);
        }
        for (int p = p0 + wave; p < p1; p += 4) {   // larger pairs: a wave each (wave-uniform)
            const uint32_t pw = s_pw[p - p0];
            const int ni = s_pn[(pw >> 15) & 63], nj = s_pn[(pw >> 21) & 63], cells = (ni + 1) * (nj + 1);
            if (cells <= 64) continue;
            long long swi = 0, swj = 0, sb = 0;
            jsfs_sums(s_cells + ((int)(pw & 0x7FFFu) - base), cells, ni, nj, lane, 64, swi, swj, sb);
            swi = wave_sum_i64(swi);
            swj = wave_sum_i64(swj);
            sb = wave_sum_i64(sb);
            if (lane == 0) emit(p, swi, swj, sb, ni, nj);
        }
    }
}

template __global__ void window_jsfs_kernel<2>(DevParams, const void *, uint32_t, uint32_t, JsfsArgs);
template __global__ void window_jsfs_kernel<4>(DevParams, const void *, uint32_t, uint32_t, JsfsArgs);
template __global__ void window_jsfs_kernel<8>(DevParams, const void *, uint32_t, uint32_t, JsfsArgs);
template __global__ void window_jsfs_kernel<16>(DevParams, const void *, uint32_t, uint32_t, JsfsArgs);

hipError_t launch_window_jsfs(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                              const JsfsArgs &A, hipStream_t stream) {
    if (n_win == 0 || A.n_pairs == 0) return hipSuccess;
    const dim3 g(n_win), b(256);
    const size_t lds = (size_t)A.lds_cells * 4;
    switch (rb) {
        case 2: hipLaunchKernelGGL(window_jsfs_kernel<2>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
        case 4: hipLaunchKernelGGL(window_jsfs_kernel<4>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
        case 8: hipLaunchKernelGGL(window_jsfs_kernel<8>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
        default: hipLaunchKernelGGL(window_jsfs_kernel<16>, g, b, lds, stream, P, rows, n_rows, n_win, A); break;
    }
    return hipGetLastError();
}

}  // namespace pbg
