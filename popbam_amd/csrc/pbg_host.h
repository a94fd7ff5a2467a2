// pbg_host.h -- host-side internals of libpopbam_gpu.so (not part of the C-ABI).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/popbam_gpu.h"

namespace pbg {

void build_errmod_tables(std::vector<double> &fk, std::vector<double> &beta, std::vector<double> &lhet);
// The errmod tables are constants (errmod_init(1.0-0.83) has no input): `make` writes them once
// next to the library (errmod_tables.bin, gen_tables.cpp) and a context reads them back instead
// of recomputing ~2 M x87 expl/logl (~0.2-0.3 s of every fresh process).  Returns false (and the
// caller computes them) when the file is absent, of another layout or fails its checksum, or
// when POPBAM_TABLES=compute.
bool write_errmod_tables(const char *path);
bool load_errmod_tables(const char *path, std::vector<double> &fk, std::vector<double> &beta, std::vector<double> &lhet);
void build_sfs_constants(int n, std::vector<double> &a1, std::vector<double> &a2, std::vector<double> &e1,
                         std::vector<double> &e2);
void build_r2_table(int n_pop, std::vector<double> &t);

// The per-site tract table of a window (pbg_window_nsl, pbg_window_xpnsl): chain p has n[p] sites; site k
// at s = p * stride + k: pos[s] its contig position, 0-based, m[m_per * s ..] the derived counts,
// sl[2 * s ..] and cens[2 * s ..] the call's sums.  Empty when the caller has none (pbg_format).
struct TractTable {
    std::vector<int32_t> n, pos, m, cens;
    std::vector<int64_t> sl;
    int stride = 0;
    // whether it holds `chains` chains with m_per ints of m a site
    bool holds(size_t chains, size_t m_per) const {
        return n.size() == chains && pos.size() == chains * stride && m.size() == m_per * pos.size() &&
               sl.size() == 2 * pos.size() && cens.size() == 2 * pos.size();
    }
    // block-wide arrays of blk_stride slots a chain -> the `chains` chains from chain e0 on, rows -> positions
    void slice(const TractTable &blk, size_t e0, size_t chains, size_t m_per, int32_t pos0) {
        const size_t s0 = e0 * blk.stride, per = chains * blk.stride;
        stride = blk.stride;
        n.assign(blk.n.begin() + e0, blk.n.begin() + e0 + chains);
        pos.assign(blk.pos.begin() + s0, blk.pos.begin() + s0 + per);
        for (int32_t &x : pos)
            if (x >= 0) x += pos0;   // row -> contig position
        m.assign(blk.m.begin() + s0 * m_per, blk.m.begin() + (s0 + per) * m_per);
        cens.assign(blk.cens.begin() + s0 * 2, blk.cens.begin() + (s0 + per) * 2);
        sl.assign(blk.sl.begin() + s0 * 2, blk.sl.begin() + (s0 + per) * 2);
    }
};

// Host copies of one window's results, as print_<stat> needs them.
struct WindowHost {
    int32_t beg = 0, end = 0;       // contig coordinates [beg, end)
    int32_t num_sites = 0, segsites = 0;
    std::vector<double> pi, dxy, td, fwh, ld_val, ld_q, div_ind, div_pop, hap_val, hap_dxy;
    std::vector<int32_t> ld_snps, div_fixed, div_seg, nhaps, hap_min, tree_diff;
    // sfs --theta (pbg_cmd.output bit 0): calc_sfs's S, Watterson's theta and the spectrum
    // sfs[0..n_pop] per population (pop_sfs.cpp:246-263)
    std::vector<int32_t> seg_pop;
    std::vector<double> theta_w;
    std::vector<std::vector<int32_t>> sfs_bins;
    // ld -o 0 --decay (pbg_cmd.decay_bin > 0): pairs and r^2 sum of bin k of population p at
    // [p * decay_bins + k] (pbg_window_ld_decay); empty when the caller has none (pbg_format)
    std::vector<int64_t> decay_pairs;
    std::vector<double> decay_sum;
    // sfs --joint (pbg_cmd.output bit 1): Fst of pair p at [p], the window's packed cells
    // (pbg_window_jsfs), shaped by pop_n; empty when the caller has none (pbg_format)
    std::vector<double> jsfs_fst;
    std::vector<int32_t> jsfs_cells;
    // sfs --dstat (pbg_cmd.output bit 2): D, f_d, f_dM of triple t at [t] and its six sums at
    // [t * 6] (pbg_window_dstat over dstat_triples(np)); empty when the caller has none (pbg_format)
    std::vector<double> dstat_d, dstat_fd, dstat_fdm;
    std::vector<int64_t> dstat_sums;
    // haplo --hfs (pbg_cmd.hfs): H1, H12, H123, H2H1, Hd of population p at [p * 5], its class count
    // at hfs_k[p] and its sorted class sizes at [p * hfs_stride] (pbg_window_hfs); empty when the
    // caller has none (pbg_format)
    std::vector<double> hfs_h;
    std::vector<int32_t> hfs_k, hfs_counts;
    int hfs_stride = 0;
    // ld --rmin (PBG_LD_RMIN in pbg_cmd.output): Rm of population p at rmin_n[p] and its chosen intervals as (left,
    // right) contig positions, 0-based, at [(p * rmin_stride + k) * 2], k < rmin_n[p]
    // (pbg_window_rmin); empty when the caller has none (pbg_format)
    std::vector<int32_t> rmin_n, rmin_cuts;
    int rmin_stride = 0;
    // haplo --nsl and --xpnsl (PBG_HAPLO_NSL, PBG_HAPLO_XPNSL in pbg_cmd.output): the chains are the
    // populations, and the population pairs (i < j, lexicographic), with two ints of m a site
    TractTable nsl, xpnsl;
    // the populations' sizes, for --joint, --nsl and --xpnsl; empty when the caller has none (pbg_format)
    std::vector<int32_t> pop_n;
    // nucdiv --snn (PBG_NUCDIV_SNN in pbg_cmd.output): Snn of group e at snn_val[e] and its permutations
    // with sum_r >= sum at snn_ge[e] (pbg_window_snn over snn_groups(np)); empty when the caller has none
    // (pbg_format)
    std::vector<double> snn_val;
    std::vector<int32_t> snn_ge;
};

// nucdiv --snn's groups of n_pops populations: all of them together (first, and only with three or more),
// then every pair i < j in lexicographic order; none for one population
inline std::vector<uint64_t> snn_groups(int n_pops) {
    std::vector<uint64_t> g;
    if (n_pops >= 3) g.push_back(n_pops >= 64 ? ~0ULL : (1ULL << n_pops) - 1);
    for (int i = 0; i < n_pops; ++i)
        for (int j = i + 1; j < n_pops; ++j) g.push_back(1ULL << i | 1ULL << j);
    return g;
}

// sfs --dstat's triples of n_pops populations: all (i, j, k) with i < j and k neither, in
// lexicographic order -- n_pops * (n_pops - 1) / 2 * (n_pops - 2) of them
inline std::vector<pbg_triple> dstat_triples(int n_pops) {
    std::vector<pbg_triple> t;
    for (int i = 0; i < n_pops; ++i)
        for (int j = i + 1; j < n_pops; ++j)
            for (int k = 0; k < n_pops; ++k)
                if (k != i && k != j) t.push_back({i, j, k});
    return t;
}

// print_nucdiv / print_sfs / print_ld / print_diverge / print_haplo (TSV, byte-identical)
void format_window(std::string &out, const pbg_cmd &cmd, int n_samples, int n_pops, uint32_t flag,
                   const WindowHost &w);

// print_popbam_snp (pop_snp.cpp:224-241) for one position's consensus words
void format_snp_site(std::string &out, const pbg_cmd &cmd, int n_samples, int32_t pos, unsigned char refc,
                     const uint64_t *cb);
// sample masks of up to PBG_MAX_SAMPLES bits (the reference's u64 for n <= 64)
typedef unsigned __int128 mask128;
inline int popcount128(mask128 x) { return __builtin_popcountll((uint64_t)x) + __builtin_popcountll((uint64_t)(x >> 64)); }
void format_sweep_site(std::string &out, const pbg_cmd &cmd, int n_pops, const mask128 *pop_mask, uint32_t flag,
                       int32_t pos, mask128 types);
void format_ms_header(std::string &out, int n_samples, int n_pops, const int32_t *pop_n, long n_windows);
void format_ms_window(std::string &out, int n_samples, uint32_t flag, int outidx, int32_t wbeg, int32_t wend,
                      const std::vector<int32_t> &pos, const std::vector<mask128> &types);

}  // namespace pbg
