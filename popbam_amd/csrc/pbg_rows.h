// pbg_rows.h -- device helpers shared by the kernels that read packed rows: the sample-mask types,
// the packed-row decoder, the wave prefix sum, the window clamp and the launch switch over the row
// width.  A window's rows are walked in one of two ways, each written once here:
//   - stream_window_rows: four waves, the words dealt among them, each wave's segregating rows in
//     an LDS queue of its own (jsfs_kernel.hip, dstat_kernel.hip, hfs_kernel.hip, with the
//     per-population count batches of the first two);
//   - gather_rows_in_order: one wave, the kept rows in row order with their row indices
//     (stats_kernel.hip, and rmin_kernel.hip through stream_rows_in_order; decay_kernel.hip keeps
//     the same loop written out, for the reason given there).
#pragma once
#include <type_traits>

#include "pbg_common.h"

namespace pbg {

namespace {

__device__ __forceinline__ unsigned pc(uint64_t x) { return (unsigned)__popcll(x); }

// The sample bits of a row: one u64 for 2 / 4 / 8-byte rows, two for 16-byte rows (n <= 126;
// the reference's masks are one u64, n <= 64, popbam.cpp:168).  Every statistic is written
// once over the mask type M: a bitwise and / complement, equality, the unsigned order
// (std::list::sort in calc_ehhs), popcount and a bit test.
struct M2 {
    uint64_t lo, hi;
};
__device__ __forceinline__ M2 operator&(M2 a, M2 b) { return {a.lo & b.lo, a.hi & b.hi}; }
__device__ __forceinline__ M2 operator~(M2 a) { return {~a.lo, ~a.hi}; }
__device__ __forceinline__ bool operator==(M2 a, M2 b) { return a.lo == b.lo && a.hi == b.hi; }
__device__ __forceinline__ bool operator<(M2 a, M2 b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ unsigned pc(M2 x) { return pc(x.lo) + pc(x.hi); }
__device__ __forceinline__ bool nonzero(uint64_t x) { return x != 0; }
__device__ __forceinline__ bool nonzero(M2 x) { return (x.lo | x.hi) != 0; }
__device__ __forceinline__ uint32_t bit(uint64_t x, int v) { return (uint32_t)(x >> v) & 1u; }
__device__ __forceinline__ uint32_t bit(M2 x, int v) { return (uint32_t)(v < 64 ? x.lo >> v : x.hi >> (v - 64)) & 1u; }
template <class M>
__device__ __forceinline__ M pop_mask(const DevParams &P, int i);
template <>
__device__ __forceinline__ uint64_t pop_mask<uint64_t>(const DevParams &P, int i) { return P.pop_mask[i]; }
template <>
__device__ __forceinline__ M2 pop_mask<M2>(const DevParams &P, int i) { return {P.pop_mask[i], P.pop_mask_hi[i]}; }
template <int RB>
struct RowMask { using T = uint64_t; };
template <>
struct RowMask<16> { using T = M2; };

// exclusive wave prefix of a lane count (DPP inclusive scan, see call_kernel.hip)
__device__ __forceinline__ uint32_t wave_incl_scan_s(uint32_t v) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);
    return (uint32_t)x;
}

// Row r (0 .. 16/RB - 1) of a 16-byte word of RB-byte rows (include/popbam_gpu.h row format).
template <int RB>
__device__ __forceinline__ void row_in_word(const uint4 &q, int r, typename RowMask<RB>::T &types, bool &counted,
                                            bool &seg) {
    if constexpr (RB == 16) {
        types.lo = (uint64_t)q.x | ((uint64_t)q.y << 32);
        types.hi = ((uint64_t)q.z | ((uint64_t)q.w << 32)) & 0x3FFFFFFFFFFFFFFFULL;
        counted = (q.w >> 30) & 1u;
        seg = (q.w >> 31) & 1u;
    } else {
        const uint32_t wd[4] = {q.x, q.y, q.z, q.w};
        constexpr int W = RB * 8;
        uint64_t v;
        if constexpr (RB == 8) v = (uint64_t)wd[2 * r] | ((uint64_t)wd[2 * r + 1] << 32);
        else if constexpr (RB == 4) v = wd[r];
        else v = (wd[r >> 1] >> (16 * (r & 1))) & 0xFFFFu;
        counted = (v >> (W - 2)) & 1;
        seg = (v >> (W - 1)) & 1;
        types = v & ((W == 64) ? 0x3FFFFFFFFFFFFFFFULL : ((1ULL << (W - 2)) - 1));
    }
}

// 16-byte word c of the packed rows; the batch's last, partial word is assembled from its
// rows alone (no read past n_rows * RB bytes)
template <int RB>
__device__ __forceinline__ uint4 load_row_word(const void *rows, uint32_t n_rows, int64_t c) {
    constexpr int R = 16 / RB;
    if ((c + 1) * R <= (int64_t)n_rows) return reinterpret_cast<const uint4 *>(rows)[c];
    uint32_t wd[4] = {0, 0, 0, 0};
    const unsigned char *rb = reinterpret_cast<const unsigned char *>(rows) + c * 16;
    for (int x = 0; (int64_t)c * 16 + x < (int64_t)n_rows * RB && x < 16; x += 2)
        wd[x >> 2] |= (uint32_t)(*reinterpret_cast<const uint16_t *>(rb + x)) << (8 * (x & 3));
    return make_uint4(wd[0], wd[1], wd[2], wd[3]);
}

// the sample bits of t inside population mask pm, packed to bit positions 0..pc(pm)-1
__device__ __forceinline__ uint32_t pext32(uint64_t t, uint64_t pm, uint32_t &k) {
    uint32_t out = 0;
    while (pm) {
        const int p = __builtin_ctzll(pm);
        out |= (uint32_t)((t >> p) & 1u) << k;
        ++k;
        pm &= pm - 1;
    }
    return out;
}
__device__ __forceinline__ uint32_t compact32(uint64_t t, uint64_t pm) {
    uint32_t k = 0;
    return pext32(t, pm, k);
}
__device__ __forceinline__ uint32_t compact32(M2 t, M2 pm) {
    uint32_t k = 0;
    const uint32_t lo = pext32(t.lo, pm.lo, k);
    return lo | pext32(t.hi, pm.hi, k);
}

// ---- the row stream of the side-table kernels (jsfs_kernel.hip, dstat_kernel.hip, hfs_kernel.hip)
//
// One workgroup of four waves per window.  Every wave takes 64 consecutive 16-byte row words of the
// window at a time (wave v the words v * 64 .., then 256 words on), the next AHEAD words of each
// lane loaded ahead; it decodes them, packs the segregating rows of the window into an LDS queue
// of its own (wave prefix sum, so the queue keeps the rows' order) and hands the queue to the
// caller's body.  No list of rows outlives a trip, so there is no capacity and no workspace: a trip
// decodes at most 64 * (16 / RB) rows, which is the queue's size.

// LDS written by some lanes of a wave, read by others of the same wave
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000LL); }

// a queued row: the sample bits in the narrowest word that holds them
template <int RB>
struct QueuedRow {
    using T = uint32_t;
    __device__ __forceinline__ static T put(uint64_t t) { return (uint32_t)t; }
    __device__ __forceinline__ static uint64_t get(T q) { return q; }
};
template <>
struct QueuedRow<8> {
    using T = uint64_t;
    __device__ __forceinline__ static T put(uint64_t t) { return t; }
    __device__ __forceinline__ static uint64_t get(T q) { return q; }
};
template <>
struct QueuedRow<16> {
    using T = M2;
    __device__ __forceinline__ static T put(M2 t) { return t; }
    __device__ __forceinline__ static M2 get(T q) { return q; }
};

// the populations' masks and sizes in LDS; stage() is followed by a __syncthreads() of the caller's
struct PopLds {
    uint64_t pm[PBG_MAX_POPS], pmh[PBG_MAX_POPS];
    int32_t pn[PBG_MAX_POPS];
    __device__ __forceinline__ void stage(const DevParams &P, int tid) {
        if (tid < P.npops) {
            pm[tid] = P.pop_mask[tid];
            pmh[tid] = P.pop_mask_hi[tid];
            pn[tid] = P.pop_n[tid];
        }
    }
    template <int RB>
    __device__ __forceinline__ typename RowMask<RB>::T mask(int i) const {
        if constexpr (RB == 16) return M2{pm[i], pmh[i]};
        else return pm[i];
    }
};

// the rows [wb, we) of a window: end <= beg is an empty window, whatever its coordinates; a window
// outside the rows is empty too, reported (error bit 4: pbg_check -> PBG_E_RANGE) and never read
struct WindowRows {
    int64_t wb, we;
    bool empty;
};
__device__ __forceinline__ WindowRows clamp_window(const pbg_window &win, uint32_t n_rows, int *err, int tid) {
    const int64_t wb = win.beg, we = win.end;
    if (we > wb && wb >= 0 && we <= (int64_t)n_rows) return {wb, we, false};
    if (we > wb && tid == 0) atomicOr(err, 4);
    return {0, 0, true};
}

// The stream.  q is the calling wave's queue of 64 * (16 / RB) entries.  body(nq) runs once per
// trip that queued nq > 0 rows, q[0 .. nq) visible to every lane of the wave, and may use wave-level
// barriers: the trip count and nq are wave-uniform.  A lane past the window's last word (c >= c1)
// decodes a zero word it never loaded; the last word is loaded row by row (load_row_word).
template <int RB, int AHEAD, class Body>
__device__ __forceinline__ void stream_window_rows(const void *rows, uint32_t n_rows, const WindowRows &win, int wave,
                                                   int lane, typename QueuedRow<RB>::T *q, Body body) {
    using Q = QueuedRow<RB>;
    constexpr int R = 16 / RB;
    const int64_t wb = win.wb, we = win.we, c0 = wb / R, c1 = (we + R - 1) / R;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    uint4 nx[AHEAD];
#pragma unroll
    for (int a = 0; a < AHEAD; ++a) {
        const int64_t c = c0 + wave * 64 + lane + 256 * a;
        nx[a] = c < c1 ? load_row_word<RB>(rows, n_rows, c) : zero;
    }
    for (int64_t cb = c0 + wave * 64; cb < c1; cb += 256) {   // wave-uniform
        const int64_t c = cb + lane;
        const uint4 w = nx[0];
        // this trip's word has arrived before the next load is issued.  Left to the compiler the wait
        // goes where the word is first used, which may be after the issue, and a wait there covers the
        // new load too (the loads are conditional, so it is vmcnt(0)) and undoes the load-ahead
        __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
        for (int a = 1; a < AHEAD; ++a) nx[a - 1] = nx[a];
        nx[AHEAD - 1] = c + 256 * AHEAD < c1 ? load_row_word<RB>(rows, n_rows, c + 256 * AHEAD) : zero;
        typename RowMask<RB>::T t[R];
        uint32_t vm = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t ri = c * R + r;
            bool cnt, sg;
            row_in_word<RB>(w, r, t[r], cnt, sg);
            vm |= (c < c1 && ri >= wb && ri < we && sg) ? (1u << r) : 0u;
        }
        const uint32_t ls = (uint32_t)__popc(vm);
        const uint32_t incl = wave_incl_scan_s(ls);
        uint32_t j = incl - ls;   // j + ls <= incl of lane 63 <= 64 * R
#pragma unroll
        for (int r = 0; r < R; ++r)
            if ((vm >> r) & 1u) q[j++] = Q::put(t[r]);
        const int nq = __builtin_amdgcn_readlane((int)incl, 63);
        if (nq == 0) continue;
        wave_sync();
        body(nq);
        wave_sync();   // the next trip's queue
    }
}

// ---- the ordered gather of one wave (stats_kernel.hip, rmin_kernel.hip)
//
// The stream above deals a window's words to four waves and keeps no row index, so it cannot hand
// one wave a window's rows in order.  Here a single wave walks the window's 16-byte words 64 at a
// time (a trip), the loads of GROUP trips issued together so that the dependent steps wait on one
// memory latency per group; a lane past the window's last word decodes a zero word it never loaded,
// and the batch's last word is loaded row by row (load_row_word).
//   keep(t, counted, seg) -> bool  runs once for every row of the window, in no particular order,
//                                  and may narrow the row's bits t.  It also runs, without a branch,
//                                  for the other rows of the decoded words: those come as neither
//                                  counted nor segregating and are never kept, so a keep that acts
//                                  on its flags alone sees the window's rows and nothing else;
//   put(j, t, row)                 runs for every kept row: j is its rank among the trip's kept
//                                  rows, in row order (j < 64 * (16 / RB)), row its absolute index;
//   trip(nq)                       runs after each trip, nq its kept rows; the trip count and nq
//                                  are wave-uniform, so trip may use wave-level barriers.
template <int RB, int GROUP, class Keep, class Put, class Trip>
__device__ __forceinline__ void gather_rows_in_order(const void *rows, uint32_t n_rows, const WindowRows &win, int lane,
                                                     Keep keep, Put put, Trip trip) {
    constexpr int R = 16 / RB;
    const int64_t wb = win.wb, we = win.we, c0 = wb / R, c1 = (we + R - 1) / R;
    uint4 qa[GROUP];
    for (int64_t cg = c0; cg < c1; cg += 64 * GROUP) {   // wave-uniform
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
            const int64_t c = cg + 64 * u + lane;
            qa[u] = c < c1 ? load_row_word<RB>(rows, n_rows, c) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < GROUP; ++u) {
            const int64_t cb = cg + 64 * u;
            if (cb >= c1) break;   // wave-uniform
            const int64_t c = cb + lane;
            typename RowMask<RB>::T t[R];
            uint32_t vm = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int64_t ri = c * R + r;
                const bool in = c < c1 && ri >= wb && ri < we;
                bool cnt, sg;
                row_in_word<RB>(qa[u], r, t[r], cnt, sg);
                vm |= (keep(t[r], in && cnt, in && sg) && in) ? (1u << r) : 0u;
            }
            const uint32_t ls = (uint32_t)__popc(vm);
            const uint32_t incl = wave_incl_scan_s(ls);
            uint32_t j = incl - ls;   // j + ls <= incl of lane 63 <= 64 * R
#pragma unroll
            for (int r = 0; r < R; ++r)
                if ((vm >> r) & 1u) put(j++, t[r], c * R + r);
            trip((uint32_t)__builtin_amdgcn_readlane((int)incl, 63));
        }
    }
}

// The gather as a stream (rmin_kernel.hip): keep(t) decides whether a segregating row of the window
// is queued; body(nq) runs once per trip that queued nq > 0 rows and sees qx[0 .. nq) and
// qrow[0 .. nq), the kept rows' bits and absolute row indices in row order, under the rules of
// stream_window_rows.  A trip queues at most 64 * (16 / RB) rows, which is the queues' size.
template <int RB, int GROUP, class Keep, class Body>
__device__ __forceinline__ void stream_rows_in_order(const void *rows, uint32_t n_rows, const WindowRows &win, int lane,
                                                     typename QueuedRow<RB>::T *qx, int32_t *qrow, Keep keep, Body body) {
    using M = typename RowMask<RB>::T;
    gather_rows_in_order<RB, GROUP>(
        rows, n_rows, win, lane, [&](M &t, bool, bool sg) { return sg && keep(t); },
        [&](uint32_t j, const M &t, int64_t row) {
            qx[j] = QueuedRow<RB>::put(t);
            qrow[j] = (int32_t)row;
        },
        [&](uint32_t nq) {
            if (nq == 0) return;
            wave_sync();
            body((int)nq);
            wave_sync();   // the next trip's queue
        });
}

// jsfs and dstat: the per-population counts of the queued rows, kCntBytes / n_pops rows (>= 16) at
// a time.  Per batch, (row, population) items form each count once -- popcount within the mask,
// flipped (n - count) when the outgroup carries the derived allele -- and park it as a byte at
// cnt[row * n_pops + population]; then every lane of the wave runs batch(nb) over the nb rows' bytes.
constexpr int kCntBytes = 1024;   // per wave
template <int RB, class Batch>
__device__ __forceinline__ void count_batches(const typename QueuedRow<RB>::T *q, int nq, const PopLds &pops, int np,
                                              int outidx, int lane, uint8_t *cnt, Batch batch) {
    const int rows_per = kCntBytes / np;
    for (int b0 = 0; b0 < nq; b0 += rows_per) {
        if (b0) wave_sync();   // the previous batch's readers
        const int nb = nq - b0 < rows_per ? nq - b0 : rows_per;
        for (int k = lane; k < nb * np; k += 64) {
            const int row = k / np, i = k - row * np;
            const auto tt = QueuedRow<RB>::get(q[b0 + row]);
            int f = (int)pc(tt & pops.mask<RB>(i));
            if (outidx >= 0 && bit(tt, outidx)) f = pops.pn[i] - f;
            cnt[k] = (uint8_t)f;
        }
        wave_sync();
        batch(nb);
    }
}

}  // namespace

// launches f with the row width as a compile-time constant: f(std::integral_constant<int, RB>)
template <class F>
void dispatch_rb(int rb, F f) {
    switch (rb) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}

}  // namespace pbg
