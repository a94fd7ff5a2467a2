// pbg_rows.h -- device helpers shared by the statistics kernels (stats_kernel.hip,
// decay_kernel.hip): the sample-mask types, the packed-row decoder and the wave prefix sum.
#pragma once
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

}  // namespace

}  // namespace pbg
