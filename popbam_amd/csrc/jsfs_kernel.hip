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
// the window's segregating rows come through the row stream and every queued row's per-population
// counts through the count batches (both in pbg_rows.h).  The work is flat item lists, so that no
// lane idles behind another lane's row: after the (row, population) items of a batch, (row, pair)
// items read two bytes and bump one cell with an integer LDS atomic.  Integer atomics are
// order-free: two runs give the same bytes.  After a group's rows: the cells are copied out, the three sums are int64 sums of cell * weight (a
// lane per pair of up to 64 cells, a wave per larger pair with an integer butterfly) and one lane
// per pair forms Fst.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_jsfs = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

__device__ __forceinline__ long long wave_sum_i64(long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Hudson's estimator as a ratio of sums (include/popbam_gpu.h); the unit is built with
// -ffp-contract=off, so the product and the sums stay separate IEEE operations
__device__ __forceinline__ double jsfs_fst(long long swi, long long swj, long long sb, int ni, int nj) {
    if (ni < 2 || nj < 2 || sb == 0) return quiet_nan();
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
    using Q = QueuedRow<RB>;
    extern __shared__ __align__(16) unsigned char sm[];
    int32_t *s_cells = reinterpret_cast<int32_t *>(sm);
    __shared__ typename Q::T s_q[4][64 * (16 / RB)];
    __shared__ uint8_t s_cnt[4][kCntBytes];
    __shared__ PopLds s_pop;
    __shared__ uint32_t s_pw[PBG_MAX_POPS * (PBG_MAX_POPS - 1) / 2];   // the group's pair words
    const int np = P.npops, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t w = blockIdx.x;
    if (w >= n_win) return;
    s_pop.stage(P, tid);
    const int32_t *s_pn = s_pop.pn;
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, tid);

    for (int g = 0; g < A.n_groups; ++g) {
        const int p0 = A.groups[g], p1 = A.groups[g + 1], npg = p1 - p0;
        const int base = (int)(A.pairs[p0] & 0x7FFFu);
        const int ncell = (p1 < A.n_pairs ? (int)(A.pairs[p1] & 0x7FFFu) : A.n_cells) - base;
        __syncthreads();   // the masks; the previous group's readers
        for (int k = tid; k < ncell; k += 256) s_cells[k] = 0;
        for (int k = tid; k < npg; k += 256) s_pw[k] = A.pairs[p0 + k];   // off the row loop's dependent chain
        __syncthreads();

        // ---- the window's rows (pbg_rows.h): one word loaded ahead
        stream_window_rows<RB, 1>(rows, n_rows, win, wave, lane, s_q[wave], [&](int nq) {
            count_batches<RB>(s_q[wave], nq, s_pop, np, A.outidx, lane, s_cnt[wave], [&](int nb) {
                // (row, pair of this group): one cell each
                for (int k = lane; k < nb * npg; k += 64) {
                    const int row = k / npg, pr = k - row * npg;
                    const uint32_t pw = s_pw[pr];
                    const int i = (int)(pw >> 15) & 63, jj = (int)(pw >> 21) & 63;
                    const int a = s_cnt[wave][row * np + i], b = s_cnt[wave][row * np + jj];
                    const int idx = (int)(pw & 0x7FFFu) - base + a * (s_pn[jj] + 1) + b;
                    if ((uint32_t)idx < (uint32_t)ncell) atomicAdd(&s_cells[idx], 1);
                }
            });
        });
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

hipError_t launch_window_jsfs(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                              const JsfsArgs &A, hipStream_t stream) {
    if (n_win == 0 || A.n_pairs == 0) return hipSuccess;
    const dim3 g(n_win), b(256);
    const size_t lds = (size_t)A.lds_cells * 4;
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_jsfs_kernel<decltype(RB)::value>, g, b, lds, stream, P, rows, n_rows, n_win, A);
    });
    return hipGetLastError();
}

}  // namespace pbg
