// snn_kernel.hip -- the exact sample-by-sample difference matrix of a window and Hudson's nearest-neighbour
// statistic Snn (Hudson 2000) with its permutation test on gfx950, per window and group of populations
// (pbg_window_snn; no reference counterpart, DESIGN.md "Snn").
//
// window_pairdiff_kernel: one workgroup of four waves per window over the row stream (pbg_rows.h).  A
// wave stages the rows its trips queue and settles them 64 * R at a time (R = 16 / row bytes): it turns
// them, 64 at a time, into one u64 bitplane per sample (a ballot per sample; bit j of plane s = sample s
// carries the derived allele at staged row j), parks the planes in LDS and strides its lanes over the
// sample pairs: d(u, v) += popcount(plane_u ^ plane_v), summed over the settling's chunks and added to
// the window's int32 pair array in LDS with one integer atomic per pair and settling.  Integer atomics
// are order-free, so two runs give the same bytes.  LDS: the pair sums (4 bytes a pair) and the pair
// table (u | v << 8, 2 bytes a pair) are dynamic -- 47,250 bytes at 126 samples, where the four row
// queues (4 KiB), staging buffers (8 KiB) and plane sets (4 KiB) bring a launch to 63,634 bytes; with
// narrower rows the queues and staging are 12 to 24 KiB and the pairs at most 11,346 bytes.
//
// window_snn_kernel: one workgroup per (window, group, chunk of permutations).  It reads the group's part
// of the matrix once and keeps, per member a, the nearest-neighbour set as a bitmask over member indices
// (two u64), T_a (as an index into the ascending list of distinct T values) and the true label; every
// chunk forms the observed sum (integers, then one ordered double sum: the same bits in every
// workgroup), chunk 0 stores it.  A wave then runs 64 / N' permutations side by side (N' = N rounded up
// to a power of two; above 64 members one permutation, two members a lane), a lane per member:
//   key     mix(pr + (sample + 1) G), stored to the wave's LDS;
//   rank    the count of the permutation's members with a smaller (key, index): N broadcast LDS reads;
//   label   the true label of the member with that index; the per-label member masks of the permuted
//           labelling are built with 64-bit LDS ors;
//   W_a     popcount(NN_a & mask[label_a]), added to bucket T_a with an integer LDS add;
//   sum_r   one lane per permutation walks the distinct T values in ascending order and compares.
// The counts of sum_r >= sum are added up per workgroup and reach ge with one integer global add; the
// call zeroes ge first.  No workspace, no floating-point atomic, no scratch.
#include "pbg_common.h"
#include "pbg_rows.h"

namespace pbg {
extern const int kBuildKind_snn = PBG_BUILD_KIND;   // pbg_build_info()
}

namespace pbg {

namespace {

constexpr int kSnnSlots = 128;   // PBG_MAX_SAMPLES rounded up: members, keys, buckets

__device__ __forceinline__ uint64_t snn_mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
constexpr uint64_t kSnnG = 0x9E3779B97F4A7C15ULL;

__device__ __forceinline__ void lds_or64(uint64_t *p, uint64_t v) {
    atomicOr(reinterpret_cast<unsigned long long *>(p), (unsigned long long)v);
}

// the ordered sum over the distinct T values: S_t / t, ascending t, from +0.0 (the unit is built with
// -ffp-contract=off; an empty bucket would add +0.0 and is skipped)
__device__ __forceinline__ double snn_sum(const int32_t *S, const int32_t *tval, int nT) {
    double sum = 0.0;
    for (int k = 0; k < nT; ++k) {
        const int32_t s = S[k];
        if (s != 0) sum += (double)s / (double)tval[k];
    }
    return sum;
}

}  // namespace

template <int RB>
__global__ __launch_bounds__(256) void window_pairdiff_kernel(DevParams P, const void *__restrict__ rows, uint32_t n_rows,
                                                              uint32_t n_win, SnnArgs A) {
    using M = typename RowMask<RB>::T;
    using Q = QueuedRow<RB>;
    constexpr int R = 16 / RB;
    extern __shared__ __align__(16) unsigned char s_pd[];
    __shared__ typename Q::T s_q[4][64 * R];
    __shared__ typename Q::T s_st[4][128 * R];   // the rows staged for the next settling
    __shared__ uint64_t s_pl[4][kSnnSlots];     // sample s, chunk c of the settling at s * R + c (n * R <= 128)
    const int n = P.n, npairs = A.n_pairs, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    int32_t *s_acc = reinterpret_cast<int32_t *>(s_pd);
    uint16_t *s_uv = reinterpret_cast<uint16_t *>(s_acc + npairs);
    const uint32_t w = blockIdx.x;
    if (w >= n_win) return;
    const WindowRows win = clamp_window(A.wins[w], n_rows, A.err, tid);

    // the pair table in the output's order: q = u (2n - u - 1) / 2 + (v - u - 1), u < v
    {
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
        if (tid < npairs) advance(tid);
        for (int q = tid; q < npairs; q += 256) {
            if (PBG_STORE_OK(A.err, q, npairs, npairs, kErrPool)) {
                s_uv[q] = (uint16_t)((uint32_t)u | (uint32_t)v << 8);
                s_acc[q] = 0;
            }
            if (q + 256 < npairs) advance(256);
        }
    }
    __syncthreads();

    // rows [0, cnt) of the wave's staging buffer, cnt <= 64 * R: their planes, then every pair's sum
    uint64_t *pl = s_pl[wave];
    typename Q::T *stage = s_st[wave];
    auto settle = [&](int cnt) {
        const int nch = (cnt + 63) >> 6;   // wave-uniform, <= R
        for (int c = 0; c < nch; ++c) {
            const int j = c * 64 + lane;
            const M t = j < cnt ? Q::get(stage[j]) : M{};
            uint64_t m0 = 0, m1 = 0;
            for (int s = 0; s < n; ++s) {   // wave-uniform
                const uint64_t b = __ballot(bit(t, s) != 0u);
                if ((s & 63) == lane) {
                    if (s < 64) m0 = b;
                    else m1 = b;
                }
            }
            if (lane < n && PBG_STORE_OK(A.err, lane * R + c, kSnnSlots, kSnnSlots, kErrPool)) pl[lane * R + c] = m0;
            if (64 + lane < n && PBG_STORE_OK(A.err, (64 + lane) * R + c, kSnnSlots, kSnnSlots, kErrPool))
                pl[(64 + lane) * R + c] = m1;
        }
        wave_sync();
        for (int q = lane; q < npairs; q += 64) {
            const uint32_t e = s_uv[q];
            const uint64_t *pu = pl + (e & 255u) * R, *pv = pl + (e >> 8) * R;
            int32_t d = 0;
            for (int c = 0; c < nch; ++c) d += (int32_t)pc(pu[c] ^ pv[c]);
            if (d != 0) atomicAdd(&s_acc[q], d);
        }
        wave_sync();   // the planes and the staged rows are free again
    };
    // A trip of the stream queues few rows where few sites segregate (64 words hold about four such rows
    // of 96 samples), and the planes and the pair loop cost the same for 4 rows as for 64: so the queued
    // rows are staged, and settled 64 * R at a time
    int ns = 0;   // wave-uniform: rows staged, < 64 * R between trips
    if (!win.empty)
        stream_window_rows<RB, 1>(rows, n_rows, win, wave, lane, s_q[wave], [&](int nq) {
            for (int j = lane; j < nq; j += 64)
                if (PBG_STORE_OK(A.err, ns + j, 128 * R, 128 * R, kErrPool)) stage[ns + j] = s_q[wave][j];
            ns += nq;
            wave_sync();
            if (ns >= 64 * R) {
                settle(64 * R);
                ns -= 64 * R;
                for (int j = lane; j < ns; j += 64) stage[j] = stage[64 * R + j];   // ns < 64 * R: no overlap
                wave_sync();
            }
        });
    if (ns > 0) settle(ns);
    __syncthreads();

    int32_t *o = A.diff + (size_t)w * (size_t)npairs;
    for (int q = tid; q < npairs; q += 256)
        if (PBG_STORE_OK(A.err, (size_t)w * (size_t)npairs + (size_t)q, (size_t)n_win * (size_t)npairs,
                         (size_t)n_win * (size_t)npairs, kErrPool))
            o[q] = s_acc[q];
}

__global__ __launch_bounds__(256) void window_snn_kernel(DevParams P, uint32_t n_win, SnnArgs A) {
    __shared__ uint8_t s_id[kSnnSlots], s_lab[kSnnSlots], s_ti[kSnnSlots];   // per member: sample, label, index of T
    __shared__ uint64_t s_nn[kSnnSlots][2];                                    // per member: the nearest neighbours
    __shared__ int32_t s_tval[kSnnSlots], s_tflag[kSnnSlots];                  // the distinct T values; T -> its index
    __shared__ int32_t s_S[kSnnSlots];                                         // the observed buckets
    __shared__ uint64_t s_tm[64][2];                                           // the true labelling's member masks
    __shared__ uint64_t s_bal[3];                                              // members 0..63, 64..127; populations with samples
    __shared__ int32_t s_cnt[4];                                               // nT, sum W, sum T, ge of this workgroup
    __shared__ double s_sum;
    __shared__ uint64_t s_key[4][kSnnSlots];                                   // per wave: the permutations' keys,
    __shared__ uint64_t s_pm[4][64][2];                                        //   member masks
    __shared__ int32_t s_pS[4][kSnnSlots];                                     //   and buckets
    const int n = P.n, np = P.npops, ng = A.n_groups, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint64_t bid = blockIdx.x;
    const int ck = (int)(bid % (uint64_t)A.chunks);
    const uint64_t we = bid / (uint64_t)A.chunks;   // element (window, group)
    if (we >= (uint64_t)n_win * (uint64_t)ng) return;   // the whole workgroup
    const uint32_t w = (uint32_t)(we / (uint64_t)ng);
    const int e = (int)(we - (uint64_t)w * (uint64_t)ng);
    const uint64_t gm = A.groups[e];
    const int32_t *dw = A.diff + (size_t)w * (size_t)A.n_pairs;

    // ---- the members, in ascending sample id, with their labels (the rank of the population among the
    // group's populations that have samples: fewer labels than members)
    int pop = -1;
    bool mem = false;
    if (tid < n) {
        pop = P.sample_pop[tid];
        mem = pop >= 0 && ((gm >> pop) & 1ULL) != 0;
    }
    const uint64_t bal = __ballot(mem);
    if (wave < 2 && lane == 0) s_bal[wave] = bal;
    if (wave == 2) {
        const uint64_t ne = __ballot(lane < np && P.pop_n[lane < np ? lane : 0] > 0);
        if (lane == 0) s_bal[2] = ne;
    }
    if (tid < kSnnSlots) {
        s_tflag[tid] = 0;
        s_S[tid] = 0;
        s_tm[tid >> 1][tid & 1] = 0;
    }
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();
    const int N = (int)(pc(s_bal[0]) + pc(s_bal[1]));
    const uint64_t gpm = gm & s_bal[2];
    const int gp = (int)pc(gpm);   // labels: gp <= N
    if (mem) {
        const int a = (wave == 0 ? 0 : (int)pc(s_bal[0])) + (int)pc(bal & ((1ULL << lane) - 1));
        if (PBG_STORE_OK(A.err, a, kSnnSlots, kSnnSlots, kErrPool)) {
            s_id[a] = (uint8_t)tid;
            s_lab[a] = (uint8_t)pc(gpm & ((1ULL << pop) - 1));
        }
    }
    __syncthreads();

    // ---- per member: the least distance, its ties and which members they are
    int T = 0;
    uint64_t nlo = 0, nhi = 0;
    if (tid < N) {
        const int sa = s_id[tid];
        int32_t mn = 0x7FFFFFFF;
        for (int b = 0; b < N; ++b) {
            if (b == tid) continue;
            const int sb = s_id[b], u = sa < sb ? sa : sb, v = sa < sb ? sb : sa;
            const int32_t d = dw[u * (2 * n - u - 1) / 2 + (v - u - 1)];
            if (d < mn) {
                mn = d;
                T = 0;
                nlo = nhi = 0;
            }
            if (d == mn) {
                ++T;
                if (b < 64) nlo |= 1ULL << b;
                else nhi |= 1ULL << (b - 64);
            }
        }
        s_nn[tid][0] = nlo;
        s_nn[tid][1] = nhi;
        s_tflag[T] = 1;   // T <= N - 1 < kSnnSlots
        lds_or64(&s_tm[s_lab[tid]][tid >> 6], 1ULL << (tid & 63));
    }
    __syncthreads();
    if (tid == 0) {
        int nT = 0;
        for (int t = 1; t < N; ++t)
            if (s_tflag[t]) {
                s_tval[nT] = t;
                s_tflag[t] = nT++;
            }
        s_cnt[0] = nT;
    }
    __syncthreads();
    const int nT = s_cnt[0];

    // ---- the observed statistic (every chunk: the permutations compare with it)
    if (tid < N) {
        const int lab = s_lab[tid], ti = s_tflag[T];
        s_ti[tid] = (uint8_t)ti;
        const int W = (int)(pc(nlo & s_tm[lab][0]) + pc(nhi & s_tm[lab][1]));
        if (W) atomicAdd(&s_S[ti], W);
        atomicAdd(&s_cnt[1], W);
        atomicAdd(&s_cnt[2], T);
    }
    __syncthreads();
    if (tid == 0) {
        const double sum = snn_sum(s_S, s_tval, nT);
        s_sum = sum;
        if (ck == 0 && PBG_STORE_OK(A.err, we, (uint64_t)n_win * (uint64_t)ng, (uint64_t)n_win * (uint64_t)ng, kErrPool)) {
            if (A.snn) A.snn[we] = sum / (double)N;
            if (A.near) {
                A.near[2 * we] = s_cnt[1];
                A.near[2 * we + 1] = s_cnt[2];
            }
        }
    }
    __syncthreads();
    if (!A.ge) return;   // the whole workgroup
    const double sum_obs = s_sum;

    // ---- this chunk's permutations: `slots` side by side in a wave, a lane per member
    int stride = 2;
    while (stride < N && stride < 64) stride <<= 1;
    const int slots = 64 / stride, slot = lane / stride, a0 = lane - slot * stride;
    const int r_beg = ck * A.per_chunk, r_end = r_beg + A.per_chunk < A.n_perms ? r_beg + A.per_chunk : A.n_perms;
    const uint32_t K = A.key0 + (uint32_t)A.wins[w].beg;
    const uint64_t base = snn_mix(((uint64_t)A.seed << 32) | (uint64_t)K);
    // a lane's one or two members
    int ma[2], mid[2], mti[2];
    uint64_t mlo[2], mhi[2];
    bool mv[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        ma[k] = a0 + 64 * k;
        mv[k] = ma[k] < N && (k == 0 || stride == 64);
        const int a = mv[k] ? ma[k] : 0;
        mid[k] = s_id[a];
        mti[k] = s_ti[a];
        mlo[k] = s_nn[a][0];
        mhi[k] = s_nn[a][1];
    }
    uint64_t *key = s_key[wave];
    int32_t *pS = s_pS[wave];
    int32_t cnt = 0;
    for (int r0 = r_beg + wave * slots; r0 < r_end; r0 += 4 * slots) {   // wave-uniform
        const int r = r0 + slot;
        const bool act = r < r_end;
        const uint64_t pr = snn_mix(base + (uint64_t)(r + 1) * kSnnG);
        pS[lane] = 0;
        pS[lane + 64] = 0;
        s_pm[wave][lane][0] = 0;
        s_pm[wave][lane][1] = 0;
        uint64_t mk[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (mv[k]) {
                mk[k] = snn_mix(pr + (uint64_t)(mid[k] + 1) * kSnnG);
                if (PBG_STORE_OK(A.err, slot * stride + ma[k], kSnnSlots, kSnnSlots, kErrPool)) key[slot * stride + ma[k]] = mk[k];
            }
        wave_sync();
        int lab[2] = {0, 0};
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (mv[k]) {
                int rank = 0;
                const uint64_t *kb = key + slot * stride;
                for (int b = 0; b < N; ++b) {
                    const uint64_t x = kb[b];
                    rank += (x < mk[k] || (x == mk[k] && b < ma[k])) ? 1 : 0;
                }
                lab[k] = s_lab[rank];
                if (act && PBG_STORE_OK(A.err, slot * gp + lab[k], 64, 64, kErrPool))
                    lds_or64(&s_pm[wave][slot * gp + lab[k]][ma[k] >> 6], 1ULL << (ma[k] & 63));
            }
        wave_sync();
#pragma unroll
        for (int k = 0; k < 2; ++k)
            if (mv[k] && act) {
                const uint64_t *m = s_pm[wave][slot * gp + lab[k]];
                const int W = (int)(pc(mlo[k] & m[0]) + pc(mhi[k] & m[1]));
                if (W && PBG_STORE_OK(A.err, slot * nT + mti[k], kSnnSlots, kSnnSlots, kErrPool))
                    atomicAdd(&pS[slot * nT + mti[k]], W);
            }
        wave_sync();
        if (a0 == 0 && act) cnt += snn_sum(pS + slot * nT, s_tval, nT) >= sum_obs ? 1 : 0;
        wave_sync();   // the next permutations' tables
    }
    if (cnt) atomicAdd(&s_cnt[3], cnt);
    __syncthreads();
    if (tid == 0 && s_cnt[3] &&
        PBG_STORE_OK(A.err, we, (uint64_t)n_win * (uint64_t)ng, (uint64_t)n_win * (uint64_t)ng, kErrPool))
        atomicAdd(&A.ge[we], s_cnt[3]);
}

int snn_chunks(uint32_t n_win, int n_groups, int n_perms) {
    if (n_perms <= 0 || n_groups <= 0 || n_win == 0) return 1;
    const uint64_t elems = (uint64_t)n_win * (uint64_t)n_groups;
    const uint64_t want = (kSnnWorkgroups + elems - 1) / elems;           // a few thousand workgroups
    const uint64_t most = ((uint64_t)n_perms + kSnnMinPerms - 1) / kSnnMinPerms;   // a chunk repays its set-up
    const int chunks = (int)(want < most ? want : most);
    const int per = (n_perms + chunks - 1) / chunks;
    return (n_perms + per - 1) / per;
}

hipError_t launch_window_pairdiff(int rb, const DevParams &P, const void *rows, uint32_t n_rows, uint32_t n_win,
                                  const SnnArgs &A, hipStream_t stream) {
    if (n_win == 0 || A.n_pairs == 0) return hipSuccess;
    if (P.n * (16 / rb) > kSnnSlots) return hipErrorInvalidValue;   // never: a row holds 8 * rb - 2 samples
    const dim3 g(n_win), b(256);
    const size_t lds = ((size_t)A.n_pairs * 6 + 15) & ~(size_t)15;
    dispatch_rb(rb, [&](auto RB) {
        hipLaunchKernelGGL(window_pairdiff_kernel<decltype(RB)::value>, g, b, lds, stream, P, rows, n_rows, n_win, A);
    });
    return hipGetLastError();
}

hipError_t launch_window_snn(const DevParams &P, uint32_t n_win, const SnnArgs &A, hipStream_t stream) {
    if (n_win == 0 || A.n_groups == 0) return hipSuccess;
    const uint64_t blocks = (uint64_t)n_win * (uint64_t)A.n_groups * (uint64_t)A.chunks;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;   // never: the caller checked
    hipLaunchKernelGGL(window_snn_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, P, n_win, A);
    return hipGetLastError();
}

}  // namespace pbg
