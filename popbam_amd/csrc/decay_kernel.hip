// decay_kernel.hip -- LD decay on gfx950: r^2 binned by the distance between sites, per window
// and population (pbg_window_ld_decay; no reference counterpart, DESIGN.md "LD decay").
//
// A chain is one (window, population).  Its variable sites v_0 < v_1 < ... are the window's
// segregating rows whose derived count m in the population has min_freq <= m <= n - min_freq
// (calc_zns's test, pop_ld.cpp:201-252).  Pair (a, b), a < b, at distance d = v_b - v_a falls in
// bin (d - 1) / bin_bp; pairs[k] counts bin k's pairs and r2_sum[k] is their r^2 (the host table
// ZnS reads) summed in pair order -- a ascending, then b ascending -- from +0.0.
//
// One workgroup per chain, one lane per bin (64 bins per wave).  Wave 0 gathers the chain's list
// (mask, row - beg) from the rows with a wave-ordered compaction, into LDS or, past kDecayCap
// sites, into a slice of the statistics workspace.  Then lane k walks a = 0 .. V-1 with two
// pointers that only move forward -- the first b at distance >= k bin_bp + 1 and the first at
// distance >= (k + 1) bin_bp + 1 -- and adds r^2(a, b) of the b between them to a register: the
// definition's order, no cross-lane reduction, no atomics on doubles, so two runs give the same
// bits.  A lane's work is (pairs in its bin) + O(V); one very wide bin is a ZnS-length chain in
// one lane (correct, slow: DESIGN.md).
#include <algorithm>

#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_decay = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

// A chain's list as the population-compacted mask | popcount << 26 (x) and the row offset (y).
struct DecayCompact {
    const uint2 *e;
    using Ent = uint32_t;
    __device__ __forceinline__ uint32_t off(uint32_t j) const { return e[j].y; }
    __device__ __forceinline__ Ent ent(uint32_t j) const { return e[j].x; }
    __device__ __forceinline__ static int idx(Ent a, Ent b, int np1) {
        return (int)((a >> 26) * (uint32_t)(np1 * np1) + (b >> 26) * (uint32_t)np1) + __popc(a & b & 0x03FFFFFFu);
    }
};
// The same with raw masks (populations of more than 26 samples, two-word masks).
template <class M>
struct DecayRaw {
    const M *m;
    const uint32_t *o;
    using Ent = M;
    __device__ __forceinline__ uint32_t off(uint32_t j) const { return o[j]; }
    __device__ __forceinline__ Ent ent(uint32_t j) const { return m[j]; }
    __device__ __forceinline__ static int idx(Ent a, Ent b, int np1) {
        return ((int)pc(a) * np1 + (int)pc(b)) * np1 + (int)pc(a & b);
    }
};

// Bin [dlo, dhi) of distances: the sequential sum of r^2 over its pairs, in pair order.
template <class L>
__device__ __forceinline__ void decay_bin(const L &ls, const double *tab, int np1, uint32_t V, uint32_t dlo, uint32_t dhi,
                                          double &acc, long long &cnt) {
    uint32_t lo = 1, hi = 1;
    for (uint32_t a = 0; a + 1 < V; ++a) {
        const uint32_t oa = ls.off(a);
        const typename L::Ent ea = ls.ent(a);
        if (lo <= a) lo = a + 1;
        while (lo < V && ls.off(lo) - oa < dlo) ++lo;
        if (lo >= V) break;   // offsets ascend: no later a reaches this bin either
        if (hi < lo) hi = lo;
        while (hi < V && ls.off(hi) - oa < dhi) ++hi;
        for (uint32_t b = lo; b < hi; ++b) acc += tab[L::idx(ea, ls.ent(b), np1)];
        cnt += (long long)(hi - lo);
    }
}

constexpr unsigned long long kDecayInLds = ~0ULL, kDecayNoList = ~0ULL - 1;

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_decay_kernel(DevParams P, DevTables T, const void *__restrict__ rows,
                                                           uint32_t n_rows, uint32_t n_win, DecayArgs A) {
    using M = typename RowMask<RB>::T;
    constexpr uint64_t NW = sizeof(M) / 8;   // pool words per mask
    constexpr int R = 16 / RB;
    extern __shared__ __align__(16) unsigned char sm[];
    __shared__ uint32_t s_V;
    __shared__ unsigned long long s_off;
    const int np = P.npops, tid = (int)threadIdx.x;
    const uint32_t ch = blockIdx.x;
    const uint32_t w = ch / (uint32_t)np;
    if (w >= n_win) return;
    const int i = (int)(ch - w * (uint32_t)np);
    const int nn = P.pop_n[i], np1 = nn + 1, mf = A.min_freq;
    const int r2n = np1 * np1 * np1;
    const bool tab_lds = r2n <= kDecayR2Lds && (uint32_t)r2n * 8u <= A.tab_bytes;
    double *s_r2 = reinterpret_cast<double *>(sm);
    const double *g_r2 = T.r2 + T.r2_off[i];
    if (tab_lds)
        for (int j = tid; j < r2n; j += (int)blockDim.x) s_r2[j] = g_r2[j];
    // the list in LDS: compacted entries, or masks then offsets
    uint2 *s_ent = reinterpret_cast<uint2 *>(sm + A.tab_bytes);
    M *s_mask = reinterpret_cast<M *>(sm + A.tab_bytes);
    uint32_t *s_offs = reinterpret_cast<uint32_t *>(sm + A.tab_bytes + (size_t)kDecayCap * sizeof(M));
    const bool compact = A.compact != 0;

    if (tid < 64) {
        // ---- gather (wave 0): the chain's variable sites in row order
        const int lane = tid;
        const M pm = pop_mask<M>(P, i);
        const int64_t wb = A.wins[w].beg, we = A.wins[w].end > A.wins[w].beg ? A.wins[w].end : A.wins[w].beg;
        const int64_t c0 = wb / R, c1 = (we + R - 1) / R;
        // The ordered gather of pbg_rows.h (gather_rows_in_order), written out: through the shared
        // template this kernel's bin walk, its instructions unchanged, measured 6 % slower at 96 samples
        // (profiles/INDEX.md, "Ordered gather").  A change to the window edge, the partial last word
        // or the load grouping there is made here too.
        constexpr int kLoadAhead = 4;   // a group's loads are issued together
        auto gather = [&](auto &&store) -> uint32_t {
            uint32_t V = 0;
            uint4 qa[kLoadAhead];
            for (int64_t cg = c0; cg < c1; cg += 64 * kLoadAhead) {
#pragma unroll
                for (int u = 0; u < kLoadAhead; ++u) {
                    const int64_t c = cg + 64 * u + lane;
                    qa[u] = c < c1 ? load_row_word<RB>(rows, n_rows, c) : make_uint4(0, 0, 0, 0);
                }
#pragma unroll
                for (int u = 0; u < kLoadAhead; ++u) {
                    const int64_t cb = cg + 64 * u;
                    if (cb >= c1) break;   // wave-uniform
                    const int64_t c = cb + lane;
                    M t[R];
                    uint32_t vm = 0;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int64_t ri = c * R + r;
                        bool cnt, sg;
                        row_in_word<RB>(qa[u], r, t[r], cnt, sg);
                        t[r] = t[r] & pm;
                        const int m = (int)pc(t[r]);
                        const bool v = c < c1 && ri >= wb && ri < we && sg && m >= mf && m <= nn - mf;
                        vm |= v ? (1u << r) : 0u;
                    }
                    const uint32_t ls = (uint32_t)__popc(vm);
                    const uint32_t incl = wave_incl_scan_s(ls);
                    uint32_t j = V + incl - ls;
#pragma unroll
                    for (int r = 0; r < R; ++r)
                        if ((vm >> r) & 1u) {
                            store(j, t[r], (uint32_t)(c * R + r - wb));
                            ++j;
                        }
                    V += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                }
            }
            return V;
        };
        uint32_t V = 0;
        // the host validated the list (and caches that by pointer): a list rewritten in place with a
        // window outside the rows is reported (pbg_check -> PBG_E_RANGE), never read
        const bool outside = wb < we && (wb < 0 || we > (int64_t)n_rows);
        if (outside && lane == 0) atomicOr(A.err, 4);
        if (wb < we && !outside)
            V = gather([&](uint32_t j, M t, uint32_t off) {
                if (j >= (uint32_t)kDecayCap) return;
                if (compact) {
                    const uint32_t cm = compact32(t, pm);
                    s_ent[j] = make_uint2(cm | (uint32_t)__popc(cm) << 26, off);
                } else {
                    s_mask[j] = t;
                    s_offs[j] = off;
                }
            });
        unsigned long long off = kDecayInLds;
        if (V > (uint32_t)kDecayCap) {   // the whole list goes to a workspace slice (second pass)
            const uint64_t size = compact ? (uint64_t)V : (uint64_t)V * NW + ((uint64_t)V + 1) / 2;
            if (lane == 0) {
                off = atomicAdd(A.pool_used, (unsigned long long)size);
                if (off + size > A.pool_cap) {
                    atomicOr(A.err, 4);
                    off = kDecayNoList;
                }
            }
            off = __shfl(off, 0, 64);
            if (off == kDecayNoList) {   // pool exhausted: reported by pbg_check, the chain's outputs are zero
                V = 0;
            } else {
                uint2 *p_ent = reinterpret_cast<uint2 *>(A.pool + off);
                M *p_mask = reinterpret_cast<M *>(A.pool + off);
                uint32_t *p_offs = reinterpret_cast<uint32_t *>(A.pool + off + (uint64_t)V * NW);
                (void)gather([&](uint32_t j, M t, uint32_t o) {
                    if (compact) {
                        if (!PBG_POOL_OK(A, off + (uint64_t)j, off, size)) return;
                        const uint32_t cm = compact32(t, pm);
                        p_ent[j] = make_uint2(cm | (uint32_t)__popc(cm) << 26, o);
                    } else {
                        if (!PBG_POOL_OK(A, off + ((uint64_t)j + 1) * NW - 1, off, size) ||
                            !PBG_POOL_OK(A, off + (uint64_t)V * NW + j / 2, off, size))
                            return;
                        p_mask[j] = t;
                        p_offs[j] = o;
                    }
                });
            }
        }
        if (lane == 0) {
            s_V = V;
            s_off = off;
            if (A.n_var) A.n_var[ch] = (int32_t)V;
        }
    }
    __syncthreads();

    // ---- binning: lane k owns bin k
    const int k = tid;
    if (k >= A.n_bins) return;
    const uint32_t V = s_V;
    const unsigned long long off = s_off;
    const uint64_t dl = (uint64_t)k * (uint64_t)A.bin_bp + 1, dh = dl + (uint64_t)A.bin_bp;
    // distances are below 2^31 (row indices are int32): bounds past 2^32 - 1 compare alike
    const uint32_t dlo = dl > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dl, dhi = dh > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dh;
    double acc = 0.0;
    long long cnt = 0;
    auto run = [&](const double *tab) {
        if (off == kDecayInLds) {
            if (compact) decay_bin(DecayCompact{s_ent}, tab, np1, V, dlo, dhi, acc, cnt);
            else decay_bin(DecayRaw<M>{s_mask, s_offs}, tab, np1, V, dlo, dhi, acc, cnt);
        } else {
            const uint64_t *pl = A.pool + off;
            if (compact) decay_bin(DecayCompact{reinterpret_cast<const uint2 *>(pl)}, tab, np1, V, dlo, dhi, acc, cnt);
            else
                decay_bin(DecayRaw<M>{reinterpret_cast<const M *>(pl), reinterpret_cast<const uint32_t *>(pl + (uint64_t)V * NW)},
                          tab, np1, V, dlo, dhi, acc, cnt);
        }
    };
    if (V > 1) {
        if (tab_lds) run(s_r2);
        else run(g_r2);
    }
    const size_t o = (size_t)ch * (size_t)A.n_bins + (size_t)k;
    if (A.pairs) A.pairs[o] = (int64_t)cnt;
    if (A.r2_sum) A.r2_sum[o] = acc;
}

template __global__ void window_decay_kernel<2>(DevParams, DevTables, const void *, uint32_t, uint32_t, DecayArgs);
template __global__ void window_decay_kernel<4>(DevParams, DevTables, const void *, uint32_t, uint32_t, DecayArgs);
template __global__ void window_decay_kernel<8>(DevParams, DevTables, const void *, uint32_t, uint32_t, DecayArgs);
template __global__ void window_decay_kernel<16>(DevParams, DevTables, const void *, uint32_t, uint32_t, DecayArgs);

size_t decay_lds_bytes(int rb, const DevParams &P, DecayArgs &A) {
    int max_pop = 0;
    uint32_t tab = 0;
    for (int i = 0; i < P.npops; ++i) {
        max_pop = std::max(max_pop, P.pop_n[i]);
        const int64_t np1 = P.pop_n[i] + 1, r2n = np1 * np1 * np1;
        if (r2n <= kDecayR2Lds) tab = std::max<uint32_t>(tab, (uint32_t)r2n * 8u);
    }
    A.tab_bytes = (tab + 15u) & ~15u;
    A.compact = (max_pop <= 26 && rb != 16) ? 1 : 0;
    const size_t mask_bytes = rb == 16 ? 16 : 8;
    return A.tab_bytes + (A.compact ? (size_t)kDecayCap * 8 : (size_t)kDecayCap * (mask_bytes + 4));
}

hipError_t launch_window_decay(int rb, const DevParams &P, const DevTables &T, const void *rows, uint32_t n_rows,
                               uint32_t n_win, const DecayArgs &A, size_t lds, hipStream_t stream) {
    if (n_win == 0) return hipSuccess;
    const dim3 g(n_win * (uint32_t)P.npops), b(64u * (uint32_t)((A.n_bins + 63) / 64));
    switch (rb) {
        case 2: hipLaunchKernelGGL(window_decay_kernel<2>, g, b, lds, stream, P, T, rows, n_rows, n_win, A); break;
        case 4: hipLaunchKernelGGL(window_decay_kernel<4>, g, b, lds, stream, P, T, rows, n_rows, n_win, A); break;
        case 8: hipLaunchKernelGGL(window_decay_kernel<8>, g, b, lds, stream, P, T, rows, n_rows, n_win, A); break;
        default: hipLaunchKernelGGL(window_decay_kernel<16>, g, b, lds, stream, P, T, rows, n_rows, n_win, A); break;
    }
    return hipGetLastError();
}

}  // namespace pbg
