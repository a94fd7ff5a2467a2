/* popbam_gpu.h -- C-ABI of the MI355X-native POPBAM hot path (libpopbam_gpu.so).
 *
 * Drop-in boundary.  The reference drives its hot path through the pileup callback
 *     int (*bam_pileup_f)(uint32_t tid, uint32_t pos, int n, const bam_pileup1_t *pl, void *data)
 * (bam.h:554), registered per window with bam_plbuf_init(make_<cmd>, &t)
 * (bam_pileup.c:505-540) and implemented by make_nucdiv / make_sfs / make_ld / make_diverge /
 * make_haplo / make_snp (e.g. pop_nucdiv.cpp:136-204), each of which runs
 * popbamData::call_base (popbam.cpp:186-313) + clean_heterozygotes / segbase / qfilter
 * (pop_utils.cpp:102-201) per position and then calc_<stat> / print_<stat> per window.
 *
 * This library replaces everything after call_base's per-read loop:
 *   - the host side of the callback (reference popbam.cpp:220-287: skip is_del /
 *     is_refskip / BAM_FUNMAP, RG -> sample, keep the first max_depth reads per sample, then
 *     per read the baseQ / mapQ / N filters and the key qq<<5 | strand<<4 | base, plus the
 *     sum of mapQ^2) fills a pileup batch (pbg_pileup) with exactly the bytes SURVEY 8(d)
 *     counts: a u16 key per kept read, per (position, sample) the key count k (u8) and
 *     sum mapQ^2 (u32), per position the reference byte (libpopbam_feed.so does this);
 *   - pbg_call_sites()     = call_base from errmod_cal on (popbam.cpp:288-306) +
 *                            clean_heterozygotes + segbase + qfilter + cal_site_type + the
 *                            make_<cmd> site store, producing one packed row per position;
 *   - pbg_window_stats()   = calc_diff_matrix + calc_nucdiv / calc_sfs / calc_zns /
 *                            calc_omegamax / calc_wall / calc_diverge / calc_nhaps /
 *                            calc_ehhs / calc_minDxy over any list of windows;
 * pbg_run() chains them for one `popbam <cmd>` invocation and prints the reference's TSV
 * (print_<stat>, byte-identical); the CLI and the tests use it.
 *
 * Conventions: every entry point returns 0 on success or a negative PBG_E* code and never
 * exits; pbg_last_error() has the message.  One context per device; calls on one context are
 * not thread-safe.  Pointers documented "device" must be device (HBM) memory; the caller owns
 * all buffers it passes; the context owns its tables and scratch.  `stream` is a hipStream_t
 * (NULL = default stream); asynchronous entry points only enqueue work on it, and errors the
 * kernels detect (an inconsistent batch) are reported by the next pbg_check() on that stream.
 */
#ifndef POPBAM_GPU_H
#define POPBAM_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define PBG_MAX_SAMPLES 126    /* the reference stops at 64 (u64 masks, popbam.1:507-510,
                                  popbam.cpp:168); 65..126 use the two-word masks below and
                                  16-byte rows (126 sample bits + counted + segregating)  */
#define PBG_MAX_POPS    64     /* pop_mask[] is indexed by population (popbam.1:507-510) */
#define PBG_SITE_BLOCK  64     /* positions per pbg_pileup.block_off entry                 */

#define PBG_OK           0
#define PBG_E_ARG       -1
#define PBG_E_HIP       -2
#define PBG_E_NOMEM     -3
#define PBG_E_RANGE     -4
#define PBG_E_NODEV     -5
#define PBG_E_BATCH     -6     /* a kernel found block_off inconsistent with k[] (pbg_check) */

/* BAM_* option bits, same values as popbam.h:59-94 */
#define PBG_F_ILLUMINA     0x02
#define PBG_F_SUBSTITUTE   0x10
#define PBG_F_HETEROZYGOTE 0x20
#define PBG_F_OUTGROUP     0x40

typedef struct pbg_ctx pbg_ctx;

/* Sample model + calling filters (popbamData members, popbam.h:236-264; defaults
 * popbam.cpp:79-93). */
typedef struct {
    int32_t  n_samples;                 /* sm->n, 1..PBG_MAX_SAMPLES                     */
    int32_t  n_pops;                    /* sm->npops, 1..PBG_MAX_POPS                    */
    uint64_t pop_mask[PBG_MAX_POPS];    /* assign_pops (popbam.cpp:145-171)              */
    int32_t  pop_n[PBG_MAX_POPS];       /* pop_nsmpl                                      */
    int32_t  min_depth, max_depth;      /* -m -x                                          */
    int32_t  min_rmsQ, min_snpQ;        /* -q -s                                          */
    int32_t  min_mapQ, min_baseQ;       /* -a -b (unsigned char in the reference); applied
                                           by the host when it builds the keys            */
    uint32_t flag;                      /* PBG_F_* bits                                   */
    uint64_t pop_mask_hi[PBG_MAX_POPS]; /* samples 64..125 of each pop_mask (0 for n <= 64) */
} pbg_params;

/* Dense pileup batch for contiguous positions [pos0, pos0 + n_sites) of one contig, in the
 * layout SURVEY 8(d) prices (sum over (position, sample) of 2k + 5 bytes, + 1 per position).
 * All pointers are DEVICE pointers for pbg_call_sites, HOST pointers for pbg_run.
 *   ref[i]        reference base byte (faidx_fetch_seq); bit 7 set = the pileup made no
 *                 callback at this position (no mask-passing read covers it)
 *   k[i*n+s]      keys kept for sample s at position i: call_base's `k` after the max_depth
 *                 cap and the per-read filters (popbam.cpp:266-287); u8 when the context's
 *                 max_depth <= 255, else u16 (pbg_k_bytes)
 *   rmsq[i*n+s]   sum of mapQ^2 over those reads (popbam.cpp:287 `rmsq`)
 *   block_off[b]  index in keys[] of the first key of position b*PBG_SITE_BLOCK;
 *                 ceil(n_sites/PBG_SITE_BLOCK)+1 entries, last = total keys (pbg_run derives
 *                 it from k[] when NULL)
 *   keys[]        one u16 per kept read, (position, sample, pileup order) major:
 *                 qq<<5 | strand<<4 | base (popbam.cpp:284), qq = clamp(min(baseQ, mapQ), 4, 63)
 * Device batches: keys[], k[] and rmsq[] must be 16-byte aligned (any hipMalloc / torch
 * allocation is; the kernels read them with 16-byte loads).
 * block_off[0] need not be 0: the kernels read only the 16-byte chunks of keys[] that hold
 * keys [block_off[0], block_off[last]), so a caller may pass keys shifted back by a
 * multiple of 8 keys to address a buffer that holds only that range.                     */
typedef struct {
    uint32_t        n_sites;
    int32_t         pos0;
    const uint8_t  *ref;
    const void     *k;
    const uint32_t *rmsq;
    const uint64_t *block_off;
    const uint16_t *keys;
} pbg_pileup;

/* Row format written by pbg_call_sites: one little-endian word of W = 8*pbg_row_bytes()
 * bits per position (2 B for n<=14, 4 B for n<=30, 8 B for n<=62, 16 B for n<=126):
 *   bits 0..n-1  cal_site_type: sample derived & passing ((cb&3)==3)
 *   bit  W-2     counted: all n samples pass qfilter (popcount(sample_cov)==n)
 *   bit  W-1     segregating: counted and segbase() > 0
 * A position that is not counted has row 0.                                            */

typedef struct { int32_t beg, end; } pbg_window;   /* row index range [beg, end)           */

/* statistics selectable in pbg_window_stats */
#define PBG_S_NUCDIV   0x001   /* pi / dxy              (pop_nucdiv.cpp:206-256)      */
#define PBG_S_SFS      0x002   /* Tajima D, Fay-Wu H    (pop_sfs.cpp:227-291)         */
#define PBG_S_ZNS      0x004   /* ld -o 0               (pop_ld.cpp:201-252)          */
#define PBG_S_OMEGA    0x008   /* ld -o 1               (pop_ld.cpp:254-373)          */
#define PBG_S_WALL     0x010   /* ld -o 2               (pop_ld.cpp:375-458)          */
#define PBG_S_DIV_IND  0x020   /* diverge -o 0          (pop_diverge.cpp:228-231)     */
#define PBG_S_DIV_POP  0x040   /* diverge -o 1          (pop_diverge.cpp:232-253)     */
#define PBG_S_HAP_K    0x080   /* haplo -o 0            (pop_haplo.cpp:208-254)       */
#define PBG_S_HAP_EHHS 0x100   /* haplo -o 1            (pop_haplo.cpp:256-323)       */
#define PBG_S_HAP_DXY  0x200   /* haplo -o 2            (pop_haplo.cpp:325-363)       */
#define PBG_S_TREE     0x400   /* tree diff_matrix      (pop_tree.cpp:472-494)        */

typedef struct {
    uint32_t stats;        /* PBG_S_* mask; at most one of ZNS / OMEGA / WALL (they share
                              ld_snps / ld_val)                                            */
    int32_t  min_freq;     /* ld: 1, or 2 with -e                                         */
    int32_t  outidx;       /* sfs/diverge outgroup sample (-p) when PBG_F_OUTGROUP is set  */
    int32_t  jc;           /* diverge -d jc                                                */
} pbg_stat_opts;

/* Per-window results (DEVICE arrays, caller-allocated, NULL = not wanted).  Values are the
 * exact numbers the reference prints (already divided by num_sites where it divides). */
typedef struct {
    int32_t  *num_sites;   /* [n_win]                                                    */
    int32_t  *segsites;    /* [n_win]                                                    */
    double   *pi;          /* [n_win*n_pops]            nucdiv pi (piw/num_sites)         */
    double   *dxy;         /* [n_win*n_pops*(n_pops-1)] nucdiv dxy, reference indexing    */
    double   *td, *fwh;    /* [n_win*n_pops]            sfs                               */
    int32_t  *ld_snps;     /* [n_win*n_pops]            ld S[] column                     */
    double   *ld_val;      /* [n_win*n_pops]            ZnS / omega_max / Wall B          */
    double   *ld_q;        /* [n_win*n_pops]            Wall Q                            */
    double   *div_ind;     /* [n_win*n_samples]         diverge -o 0 distance             */
    int32_t  *div_fixed;   /* [n_win*n_pops]            diverge -o 1 Fixed (u16 wrap)     */
    int32_t  *div_seg;     /* [n_win*n_pops]            diverge -o 1 Seg                  */
    double   *div_pop;     /* [n_win*n_pops]            diverge -o 1 distance             */
    int32_t  *nhaps;       /* [n_win*n_pops]            haplo K                           */
    double   *hap_val;     /* [n_win*n_pops]            haplo Kdiv (1-hdiv) / EHHS / pi   */
    double   *hap_dxy;     /* [n_win*n_pops*(n_pops-1)] haplo -o 2 dxy                    */
    int32_t  *hap_min;     /* [n_win*n_pops*(n_pops-1)] haplo -o 2 min (u16)              */
    int32_t  *tree_diff;   /* [n_win*(n+1)*(n+1)]       tree diff_matrix (u16 values): taxon 0
                              = the reference (differences = derived count), taxon i+1 =
                              sample i; the neighbour-joining tree is built on the host      */
    /* Not printed by the reference (SURVEY 8(c) "parity unpinned"; north_star asks for them),
     * computed under PBG_S_SFS from calc_sfs's own integers (pop_sfs.cpp:227-240):           */
    int32_t  *sfs_bins;    /* [n_win*n_pops*pbg_sfs_stride()] sfs[j] = segregating sites whose
                              (outgroup-flipped) derived count in the population is j        */
    int32_t  *seg_pop;     /* [n_win*n_pops] S of calc_sfs: sites with 0 < freq < n_pop   */
    double   *theta_w;     /* [n_win*n_pops] Watterson's theta S / a1[n_pop] (a1 of
                              calc_a1, pop_sfs.cpp:511-525), per window (not per site)      */
} pbg_window_out;

/* ---- context ---------------------------------------------------------------------- */
int         pbg_create(pbg_ctx **ctx, int device, const pbg_params *params);
void        pbg_destroy(pbg_ctx *ctx);
const char *pbg_last_error(const pbg_ctx *ctx);   /* ctx may be NULL (last create error)  */
int         pbg_row_bytes(const pbg_ctx *ctx);
int         pbg_k_bytes(const pbg_ctx *ctx);      /* 1 (max_depth <= 255) or 2           */
int         pbg_sfs_stride(const pbg_ctx *ctx);   /* largest population size + 1          */
int         pbg_device_count(void);

/* ---- hot path --------------------------------------------------------------------- */
/* rows: device, n_sites * pbg_row_bytes(); cb: device u64[n_sites*n_samples] or NULL
 * (final consensus words, layout pop_utils.cpp:6-24, for the snp subcommand).           */
int pbg_call_sites(pbg_ctx *ctx, const pbg_pileup *pileup, void *rows, uint64_t *cb, void *stream);

/* The staging capacity of pbg_call_sites (from block_off's last entry) and the workspace
 * plan of pbg_window_stats (from the window list) are computed on the first call and cached
 * per (device pointer, size): steady-state calls on a resident batch enqueue kernels only.
 * A caller that rewrites a window list in place with a different layout must pass a new
 * pointer (or n_win / n_rows) to force a new plan. */
int pbg_window_stats(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                     uint32_t n_win, const pbg_stat_opts *opts, const pbg_window_out *out,
                     void *stream);

/* LD decay (an extension; the reference stops at ZnS, one number per window and population):
 * r^2 against the distance between sites.  For window [beg, end) and population i, the variable
 * sites v_0 < v_1 < ... are the window's segregating rows whose derived count m in the population
 * has min_freq <= m <= n_i - min_freq (calc_zns's test, pop_ld.cpp:201-252).  Every pair a < b
 * has distance d = v_b - v_a >= 1 and bin k = (d - 1) / bin_bp, so bin k holds distances
 * k*bin_bp + 1 .. (k + 1)*bin_bp; pairs with k >= n_bins are dropped.  pairs[k] counts bin k's
 * pairs; r2_sum[k] is the sequential double sum, from +0.0 in pair order (a ascending, then b
 * ascending), of the r^2 table entries ZnS adds -- bit for bit what a calc_zns-style double loop
 * with bin[k] += r2 gives, the same on every run; n_var is the number of variable sites (not the
 * reference's num_snps).  Windows with beg >= end and populations without variable sites give
 * zeros.  Asynchronous like pbg_window_stats, and free to interleave with it on one stream;
 * lists of more than 1024 variable sites take a slice of the statistics workspace (exhaustion:
 * pbg_check, PBG_E_RANGE).  PBG_E_ARG for bin_bp < 1, n_bins outside 1..PBG_DECAY_MAX_BINS,
 * min_freq not 1 or 2, or a null argument. */
#define PBG_DECAY_MAX_BINS 256
typedef struct { int32_t bin_bp, n_bins, min_freq, _pad; } pbg_decay_opts;
typedef struct {            /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int64_t *pairs;         /* [n_win*n_pops*n_bins] */
    double  *r2_sum;        /* [n_win*n_pops*n_bins] */
    int32_t *n_var;         /* [n_win*n_pops]        */
} pbg_decay_out;
int pbg_window_ld_decay(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                        uint32_t n_win, const pbg_decay_opts *opts, const pbg_decay_out *out, void *stream);

/* Joint site-frequency spectrum and Fst per window and population pair (an extension; between
 * populations the reference stops at dxy and the haplotype min-Dxy).  A context has populations
 * 0 .. n_pops-1 of n_i samples; the pairs are the unordered i < j, numbered lexicographically:
 * p = i*(2*n_pops - i - 1)/2 + (j - i - 1), n_pairs = n_pops*(n_pops-1)/2.  The sites of window
 * [beg, end) are its rows with the segregating bit set (the set sfs_bins is taken over).  Such a
 * row with sample bits t has a = popcount(t & pop_mask_i) and b = popcount(t & pop_mask_j); when
 * the context has PBG_F_OUTGROUP and bit outidx of t is set, both flip: a -> n_i - a, b -> n_j - b
 * (calc_sfs's flip).
 *   cells  J_p[a][b] = the window's segregating rows with counts (a, b), int32.  A window's cells
 *          are packed: pair p starts at off[p] = sum over q < p of (n_i(q)+1)*(n_j(q)+1), cell
 *          (a, b) is at off[p] + a*(n_j+1) + b, and a window's block is C = off[n_pairs] cells
 *          (pbg_jsfs_cells; at most 17,767: 64 populations over 126 samples).
 *   diffs  three int64 per (window, pair), summed over the window's segregating rows:
 *          SW_i = sum a(n_i-a), SW_j = sum b(n_j-b), SB = sum a(n_j-b) + b(n_i-a) -- the within- and
 *          between-population pairwise-difference counts; the flip leaves them unchanged.
 *   fst    Hudson's estimator as a ratio of sums, one double per (window, pair), exactly
 *              pw_i = (double)SW_i / (double)(n_i*(n_i-1)/2)
 *              pw_j = (double)SW_j / (double)(n_j*(n_j-1)/2)
 *              pb   = (double)SB   / (double)(n_i*n_j)
 *              fst  = 1.0 - (0.5 * (pw_i + pw_j)) / pb
 *          with IEEE operations and no fused multiply-add, so it is reproducible from the integers;
 *          a quiet NaN when n_i < 2, n_j < 2 or SB == 0.
 * Windows with beg >= end give zero cells, zero diffs and NaN.  n_pops == 1 is valid: PBG_OK and
 * nothing is written.  Integer atomics only, so two runs give the same bytes; no list of sites is
 * kept, so a window of any length works and the call has no workspace.  Asynchronous like
 * pbg_window_stats and free to interleave with it and with pbg_window_ld_decay on one stream (it
 * shares none of their state).  A window outside [0, n_rows] is not read: it gives the outputs of
 * an empty window and the next pbg_check returns PBG_E_RANGE.  PBG_E_ARG for a null ctx, rows,
 * wins, opts or out, for outidx outside 0..n_samples-1 when the context has PBG_F_OUTGROUP, when
 * n_win * C or n_win * n_pairs passes int32 indexing, and for a context whose pop_n[i] is not the
 * number of samples in pop_mask[i] (the cell layout is built from pop_n). */
typedef struct { int32_t outidx, _pad; } pbg_jsfs_opts;   /* the flip applies only with PBG_F_OUTGROUP */
typedef struct {               /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int32_t *cells;            /* [n_win * pbg_jsfs_cells()]  */
    int64_t *diffs;            /* [n_win * n_pairs * 3]  SW_i, SW_j, SB */
    double  *fst;              /* [n_win * n_pairs]      */
} pbg_jsfs_out;
int pbg_jsfs_cells(const pbg_ctx *ctx);                      /* C; 0 for one population (or a null ctx) */
int pbg_jsfs_pair_offset(const pbg_ctx *ctx, int i, int j);  /* off[p] for i < j; PBG_E_ARG otherwise */
int pbg_window_jsfs(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                    uint32_t n_win, const pbg_jsfs_opts *opts, const pbg_jsfs_out *out, void *stream);

/* Patterson's D (ABBA-BABA) and the windowed f_d (Martin et al. 2015) and f_dM (Malinsky et al.
 * 2015) per window and population triple (an extension).  A triple (P1, P2, P3) names three
 * distinct populations of the context, of n1, n2, n3 samples; the ancestral state comes from the
 * context's outgroup flip.  The sites of window [beg, end) are its rows with the segregating bit set
 * (the set pbg_window_jsfs and sfs_bins are taken over).  Such a row with sample bits t has
 * a = popcount(t & pop_mask_P1), b and c alike for P2 and P3; when the context has PBG_F_OUTGROUP
 * and bit outidx of t is set, all three flip: a -> n1 - a, b -> n2 - b, c -> n3 - c (calc_sfs's
 * flip).  The derived frequencies are p1 = a/n1, p2 = b/n2, p3 = c/n3.
 *   sums   six int64 per (window, triple), each the sum of an integer term over the rows named:
 *            0 ABBA  (n1-a)*b*c         all rows                          = n1*n2*n3 * (1-p1) p2 p3
 *            1 BABA  a*(n2-b)*c         all rows                          = n1*n2*n3 * p1 (1-p2) p3
 *            2 FD2   b*(b*n1 - a*n2)    rows with b*n3 >= c*n2 (donor P2) = n1*n2^2  * p2 (p2 - p1)
 *            3 FD3   c*(c*n1 - a*n3)    rows with b*n3 <  c*n2 (donor P3) = n1*n3^2  * p3 (p3 - p1)
 *            4 GD1   a*(a*n2 - b*n1)    rows with a*n3 >= c*n1 (donor P1) = n2*n1^2  * p1 (p1 - p2)
 *            5 GD3   c*(c*n2 - b*n3)    rows with a*n3 <  c*n1 (donor P3) = n2*n3^2  * p3 (p3 - p2)
 *          2 and 3 are Martin's S(P1, PD, PD, O) with PD the one of P2 and P3 of the higher derived
 *          frequency at the site (a tie goes to P2); 4 and 5 are Malinsky's -S(PD, P2, PD, O) with
 *          PD the higher of P1 and P3 (a tie goes to P1).  2 to 5 are signed.  A term stays below
 *          2^21, so no window overflows.
 *   d, fd, fdm   one double each per (window, triple), from the integers (products in int64)
 *          with exactly these IEEE operations and no fused multiply-add:
 *              num  = (double)(s0 - s1) / (double)(n1*n2*n3)
 *              den  = (double)s2 / (double)(n1*n2*n2) + (double)s3 / (double)(n1*n3*n3)
 *              den2 = (double)s4 / (double)(n2*n1*n1) + (double)s5 / (double)(n2*n3*n3)
 *              d    = (double)(s0 - s1) / (double)(s0 + s1)       a quiet NaN when s0 + s1 == 0
 *              fd   = num / den                                   a quiet NaN when den == 0.0
 *              fdm  = s0 >= s1 ? num / den : num / den2           a quiet NaN when that denominator == 0.0
 * Element (w, t) of d, fd, fdm is at w * n_triples + t, its sums at (w * n_triples + t) * 6.  Any
 * order of a triple's members is valid, and so is listing a triple more than once.  D is meaningful
 * only when none of the three populations contains the outgroup sample; such a triple is computed
 * as defined all the same.  Windows with beg >= end give zero sums and NaN.  n_triples == 0 is
 * valid: PBG_OK and nothing is written.  A NULL member of pbg_dstat_out is skipped.  Integer sums
 * only (shuffles and integer LDS atomics), so two runs give the same bytes; no list of sites is
 * kept, so a window of any length works and the call has no workspace.  The triple list is a HOST
 * array, read before the call returns; the context keeps the device copies of the lists it has
 * seen, by content.  Asynchronous like pbg_window_stats and free to interleave with it, with
 * pbg_window_ld_decay and with pbg_window_jsfs on one stream (it shares none of their state).  A
 * window outside [0, n_rows] is not read: it gives the outputs of an empty window and the next
 * pbg_check returns PBG_E_RANGE.  PBG_E_ARG for a null ctx, rows, wins, opts or out, for n_triples
 * < 0 or > PBG_DSTAT_MAX_TRIPLES, for a null triples with n_triples > 0, for a population index
 * outside 0..n_pops-1, for a triple whose three populations are not distinct, for outidx outside
 * 0..n_samples-1 when the context has PBG_F_OUTGROUP (without the flag outidx is ignored), and for a
 * context whose pop_n[i] is not the number of samples in pop_mask[i]. */
#define PBG_DSTAT_MAX_TRIPLES 4096
typedef struct { int32_t p1, p2, p3; } pbg_triple;
typedef struct { int32_t outidx, n_triples; const pbg_triple *triples; /* HOST array */ } pbg_dstat_opts;
typedef struct {               /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int64_t *sums;             /* [n_win * n_triples * 6] */
    double  *d;                /* [n_win * n_triples]     */
    double  *fd;               /* same */
    double  *fdm;              /* same */
} pbg_dstat_out;
int pbg_window_dstat(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                     uint32_t n_win, const pbg_dstat_opts *opts, const pbg_dstat_out *out, void *stream);

/* Haplotype frequency spectrum, Garud's H1, H12, H123 and H2/H1 and an unbiased haplotype diversity
 * per window and population (an extension; nhaps / hap_val of PBG_S_HAP_K stay calc_nhaps' numbers,
 * local-index quirk and integer n/(n-1) included).  The context has populations 0 .. n_pops-1;
 * population i has n_i samples and mask pm_i, and its samples in ascending sample id have local
 * indices 0 .. n_i-1.  The sites of window [beg, end) are its rows with the segregating bit set (the
 * set pbg_window_jsfs and pbg_window_dstat are taken over); the haplotype of a sample is the sequence
 * of its bit over those rows, in row order.  Two samples of a population are in the same class iff
 * their haplotypes are equal at every site of the window; the outgroup flip does not matter and is
 * not applied.  With the class sizes sorted descending, c_1 >= c_2 >= ... >= c_K (c_2 = c_3 = 0 when
 * there are fewer classes), Q = sum c_k^2 and N2 = (int64)n_i * n_i, element (w, i) at w * n_pops + i:
 *   k       int32: K, the number of classes
 *   counts  int32: c_1 .. c_K, then zeros, at (w * n_pops + i) * stride; stride = pbg_hfs_stride(),
 *           the largest population size
 *   cls     uint8 at w * n_samples + s: the local index of the lowest-id sample of s's population
 *           whose haplotype equals s's; 255 for a sample that is in no population
 *   sums    four int64: Q, c_1, c_2, c_3
 *   h       five doubles, from the integers (products in int64) with exactly these IEEE operations
 *           and no fused multiply-add:
 *               H1   = (double)Q / (double)N2
 *               H12  = (double)(Q + 2*c1*c2) / (double)N2
 *               H123 = (double)(Q + 2*(c1*c2 + c1*c3 + c2*c3)) / (double)N2
 *               H2H1 = (double)(Q - c1*c1) / (double)Q
 *               Hd   = (double)(N2 - Q) / (double)(n_i*(n_i-1))     a quiet NaN when n_i < 2
 * A non-empty window with no segregating row is one class: K = 1, c_1 = n_i, H1 = 1.  A window with
 * beg >= end gives k = 0, zero counts and sums, cls = 255 and five NaNs.  A window outside
 * [0, n_rows] is not read: it gives the empty window's outputs and the next pbg_check returns
 * PBG_E_RANGE.  A NULL member of pbg_hfs_out is skipped.  Asynchronous; no workspace and no plan, so
 * it is free to interleave with pbg_window_stats, pbg_window_ld_decay, pbg_window_jsfs and
 * pbg_window_dstat on one stream.  Integer ORs and adds only, so two runs give the same bytes; no
 * list of sites is kept, so a window of any length works.  PBG_E_ARG for a null ctx, rows, wins or
 * out and for a context whose pop_n[i] is not the number of samples in pop_mask[i].  A sample that
 * sits in two populations cannot reach this call: pbg_create refuses overlapping masks. */
typedef struct {               /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int32_t *k;                /* [n_win * n_pops]                    */
    int32_t *counts;           /* [n_win * n_pops * pbg_hfs_stride()] */
    uint8_t *cls;              /* [n_win * n_samples]                 */
    int64_t *sums;             /* [n_win * n_pops * 4]  Q, c1, c2, c3 */
    double  *h;                /* [n_win * n_pops * 5]  H1, H12, H123, H2H1, Hd */
} pbg_hfs_out;
int pbg_hfs_stride(const pbg_ctx *ctx);   /* the largest population size; 0 for a null ctx */
int pbg_window_hfs(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                   uint32_t n_win, const pbg_hfs_out *out, void *stream);

/* Hudson and Kaplan's Rm (1985), the minimum number of recombination events the four-gamete test
 * implies, and the intervals that witness them, per window and population (an extension; the
 * reference has no counterpart).  For window [beg, end) and population i (n_i samples, mask pm_i) the
 * variable sites v_0 < v_1 < ... < v_{V-1} are pbg_window_ld_decay's and ZnS's: the window's rows with
 * the segregating bit whose m = popcount(types & pm_i) has min_freq <= m <= n_i - min_freq (min_freq 1
 * or 2, ld -e), in row order.  A site's column is x = types & pm_i; a sample whose bit is clear reads
 * as ancestral, as calc_zns reads it.  Sites a < b are incompatible when x_a & x_b, x_a & ~x_b & pm_i,
 * ~x_a & x_b & pm_i and pm_i & ~(x_a | x_b) are all non-zero.  The test is symmetric under
 * complementing either column, so the outgroup plays no part, and a singleton (m = 1 or n_i - 1) is
 * never incompatible with anything.  For site b let L(b) be the largest a < b incompatible with b, if
 * any.  Walk b = 0 .. V-1 with c = 0, the right end of the last chosen interval: when L(b) exists and
 * L(b) >= c, choose the interval (v_L(b), v_b) and set c = b; two chosen intervals may share an end
 * site.  Element (w, i) at w * n_pops + i:
 *   rmin   int32: the number of chosen intervals -- the largest number of pairwise disjoint
 *          incompatible intervals, which is Hudson and Kaplan's Rm
 *   n_var  int32: V
 *   cuts   int32 pairs (left row, right row), absolute row indices, max_cuts pairs per element: the
 *          first min(rmin, max_cuts) chosen intervals in order, every remaining pair (-1, -1); rmin
 *          keeps counting past max_cuts
 * beg >= end, V < 2 and n_i < 4 give rmin = 0; rmin and cuts are the same for min_freq 1 and 2.  A
 * window outside [0, n_rows] is not read: it gives the empty window's outputs and the next pbg_check
 * returns PBG_E_RANGE.  A NULL member of pbg_rmin_out is skipped.  Asynchronous; no workspace, no plan
 * and no list of sites (the walk keeps at most n_i - 3 columns), so a window of any length
 * works and the call is free to interleave with every other window call on one stream.  Integers only:
 * two runs give the same bytes.  PBG_E_ARG for a null ctx, rows, wins, opts or out, min_freq not 1 or
 * 2, max_cuts < 0 and a non-null cuts with max_cuts == 0; n_win == 0 returns PBG_OK. */
typedef struct { int32_t min_freq, max_cuts; } pbg_rmin_opts;
typedef struct {               /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int32_t *rmin;             /* [n_win * n_pops]                */
    int32_t *n_var;            /* [n_win * n_pops]                */
    int32_t *cuts;             /* [n_win * n_pops * max_cuts * 2] */
} pbg_rmin_out;
int pbg_window_rmin(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                    uint32_t n_win, const pbg_rmin_opts *opts, const pbg_rmin_out *out, void *stream);

/* The per-site nSL tract sums (Ferrer-Admetlla et al. 2014) per window and population (an extension; the
 * reference has no counterpart).  For window [beg, end) and population i (n_i samples, mask pm_i, local
 * indices by ascending sample id) the variable sites v_0 < ... < v_{V-1} are the window's rows with the
 * segregating bit whose m = popcount(types & pm_i) has 1 <= m <= n_i - 1, in row order: exactly
 * pbg_window_rmin's list at min_freq = 1 (haplo has neither -e nor -p: no frequency cut, no outgroup
 * flip).  A site's column is x_k = types & pm_i.  A pair u < v of the population's samples agrees at k
 * when bits u and v of x_k are equal; its class there is the shared bit, 0 = the reference allele, 1 =
 * the other.  For a pair that agrees at k, l >= 1 is the number of consecutive sites k, k-1, ... at
 * which it agrees and r >= 1 the same through k, k+1, ...; its tract length at k is L = l + r - 1, the
 * number of variable sites in the maximal run of agreement that contains k, cut at the window's first
 * and last variable site.  Element (w, i) at e = w * n_pops + i has max_sites slots k:
 *   n_var  int32 [e]: V
 *   row    int32 [e * max_sites + k]: v_k as an absolute row index
 *   m      int32, same index: the derived count
 *   sl     int64 [(e * max_sites + k) * 2 + c]: the sum of L over the pairs that agree at k with class c
 *   cens   int32 [(e * max_sites + k) * 2 + s]: the agreeing pairs, both classes together, whose run
 *          reaches the window's first variable site (s = 0: l = k + 1) or its last (s = 1: r = V - k)
 * Slots k >= V hold row = -1 and zeros.  A chain with V > max_sites writes every slot as unused and still
 * reports V; nothing partial is written, and the caller reads the stride it needs from n_var.
 * max_sites = 0 is the count-only call.  The unstandardised nSL of a site, relative to the reference
 * allele, is formed by the caller (a device log is not reproducible): with P0 = (n_i-m)(n_i-m-1)/2 and
 * P1 = m(m-1)/2 it is log(((double)sl0 / (double)P0) / ((double)sl1 / (double)P1)), undefined when P0
 * or P1 is 0 and otherwise finite, since sl_c >= P_c.
 * beg >= end gives zeros.  A window outside [0, n_rows] is not read: it gives the empty window's outputs
 * and the next pbg_check returns PBG_E_RANGE.  A NULL member of pbg_nsl_out is skipped, except that the
 * backward walk reads the sites back through row: sl and cens each need row.  Asynchronous; no
 * workspace, no plan and no list of sites (one integer per sample pair, in LDS: DESIGN 3g), so a window
 * of any length works and the call is free to interleave with every other window call on one stream.
 * Integers only and no order that depends on scheduling: two runs give the same bytes.  PBG_E_ARG for a
 * null ctx, rows, wins, opts or out, max_sites < 0, a non-null row, m, sl or cens with max_sites == 0,
 * sl or cens without row, and a context whose pop_n[i] is not the number of samples in pop_mask[i];
 * n_win == 0 returns PBG_OK. */
typedef struct { int32_t max_sites, _pad; } pbg_nsl_opts;
typedef struct {               /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int32_t *n_var;            /* [n_win * n_pops]                 */
    int32_t *row;              /* [n_win * n_pops * max_sites]     */
    int32_t *m;                /* [n_win * n_pops * max_sites]     */
    int64_t *sl;               /* [n_win * n_pops * max_sites * 2] */
    int32_t *cens;             /* [n_win * n_pops * max_sites * 2] */
} pbg_nsl_out;
int pbg_window_nsl(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                   uint32_t n_win, const pbg_nsl_opts *opts, const pbg_nsl_out *out, void *stream);

/* The cross-population nSL tract sums (XP-nSL, Szpiech et al. 2021: the map-free form of XP-EHH) per
 * window and population pair (an extension; the reference has no counterpart).  Population pairs are
 * (i, j), i < j, in lexicographic order -- pbg_window_jsfs's order -- with pair index p = 0 .. n_pairs-1,
 * n_pairs = n_pops (n_pops - 1) / 2; populations are disjoint (pbg_create refuses overlapping masks).
 * For window [beg, end) and pair (i, j) the pooled sites v_0 < ... < v_{V-1} are the window's rows with
 * the segregating bit whose pooled count m = popcount(types & (pm_i | pm_j)) has 1 <= m <= n_i + n_j - 1,
 * in row order: the list pbg_window_nsl produces in a context whose single population is pm_i | pm_j, so
 * it includes the sites fixed in one of the two.  Side s = 0 is population i, side s = 1 population j.  A
 * sample pair u < v of a side agrees at k when bits u and v of types[v_k] are equal; either allele counts,
 * there are no classes.  For a pair that agrees at k, l >= 1 and r >= 1 are its runs of agreement through
 * k, k-1, ... and k, k+1, ... over the POOLED list, and its tract length is L = l + r - 1, cut at the
 * window's first and last pooled site; a pair that differs at k contributes 0.  Element (w, p) at
 * e = w * n_pairs + p has max_sites slots k:
 *   n_var  int32 [e]: V
 *   row    int32 [e * max_sites + k]: v_k as an absolute row index
 *   m      int32 [(e * max_sites + k) * 2 + s]: side s's derived count; may be 0 or n_s
 *   sl     int64, same index: the sum of L over side s's agreeing pairs
 *   cens   int32, same index: side s's agreeing pairs with l = k + 1, plus those with r = V - k (a pair
 *          that agrees across the whole window counts twice)
 * Slots k >= V hold row = -1 and zeros.  A chain with V > max_sites writes every slot as unused and still
 * reports V; nothing partial is written.  max_sites = 0 is the count-only call.  The unstandardised
 * XP-nSL of a site is formed by the caller (a device log is not reproducible): with C_s = n_s (n_s-1) / 2
 * it is log(((double)sl_0 / C_0) / ((double)sl_1 / C_1)), positive when population i carries the longer
 * tracts, undefined when C_0 or C_1 is 0 or when sl_0 or sl_1 is 0 (a side of two samples that differ at
 * the site).  beg >= end gives zeros.  A window outside [0, n_rows] is not read: it gives the empty
 * window's outputs and the next pbg_check returns PBG_E_RANGE.  A NULL member of pbg_xpnsl_out is
 * skipped, except that the backward walk reads the sites back through row: sl and cens each need row.
 * Asynchronous; no workspace, no plan and no list of sites (one integer per sample pair of the two
 * sides, in LDS: DESIGN 3h), so a window of any length works and the call is free to interleave with
 * every other window call on one stream.  Integers only and no order that depends on scheduling: two
 * runs give the same bytes.  PBG_E_ARG for a null ctx, rows, wins, opts or out, max_sites < 0, a
 * non-null row, m, sl or cens with max_sites == 0, sl or cens without row, and a context whose pop_n[i]
 * is not the number of samples in pop_mask[i]; n_win == 0 returns PBG_OK, and so does a context with one
 * population (n_pairs = 0), which writes nothing. */
typedef struct { int32_t max_sites, _pad; } pbg_xpnsl_opts;
typedef struct {               /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int32_t *n_var;            /* [n_win * n_pairs]                 */
    int32_t *row;              /* [n_win * n_pairs * max_sites]     */
    int32_t *m;                /* [n_win * n_pairs * max_sites * 2] */
    int64_t *sl;               /* [n_win * n_pairs * max_sites * 2] */
    int32_t *cens;             /* [n_win * n_pairs * max_sites * 2] */
} pbg_xpnsl_out;
int pbg_window_xpnsl(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins,
                     uint32_t n_win, const pbg_xpnsl_opts *opts, const pbg_xpnsl_out *out, void *stream);

/* The exact sample-by-sample difference matrix of a window, and Hudson's nearest-neighbour statistic Snn
 * (Hudson 2000) with its permutation test per window and group of populations (an extension; the
 * reference has no counterpart).
 *   diff   For window [beg, end) and samples u < v, d(u, v) is the number of the window's rows with the
 *          segregating bit whose bits u and v differ: a plain int32 with no 16-bit wrap (tree_diff keeps
 *          the reference's), stored at w * n(n-1)/2 + q, q = u (2n - u - 1) / 2 + (v - u - 1).
 *   groups A group is a set of at least two populations (bit i of groups[e] = population i belongs).  Its
 *          members are the samples of those populations in ascending sample id, A_0 < ... < A_{N-1},
 *          each labelled with its population.
 *   snn    For member a: m_a = min over b != a of d(A_a, A_b), T_a = #{b != a : d = m_a} and
 *          W_a = #{b != a : d = m_a and label(b) = label(a)}; T_a does not depend on the labels.  For
 *          t = 1 .. N-1, S_t = sum of W_a over the members with T_a = t, and sum = sum over t of
 *          (double)S_t / (double)t: one sequential double sum from +0.0 in ascending t, IEEE division, no
 *          contraction (terms with S_t = 0 may be skipped).  snn[w * n_groups + e] = sum / (double)N.
 *   near   near[2 (w * n_groups + e)] = sum of W_a, near[.. + 1] = sum of T_a: exact integers.
 *   ge     Permutation r = 0 .. n_perms-1 of window w: with K = (uint32_t)(key0 + (uint32_t)wins[w].beg),
 *          G = 0x9E3779B97F4A7C15, arithmetic mod 2^64 and
 *            mix(z): z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; z ^ z>>31
 *          base = mix(seed<<32 | K), pr = mix(base + (r+1) G) and key(s) = mix(pr + (s+1) G) for the
 *          absolute sample id s.  Within a group member a has rank rho(a) in the order by (key(A_a), A_a)
 *          ascending, and its permuted label is the true label of member rho(a): a group of a subset of
 *          the populations sees the order induced by the same keys (the group index is not hashed).
 *          sum_r is formed exactly as sum, and ge[w * n_groups + e] is the number of r with
 *          sum_r >= sum (double comparison); the permutation p-value is (ge + 1) / (n_perms + 1).  With
 *          n_perms = 0, ge is zero.
 * A window without a segregating row has d = 0 everywhere, so every member ties with every other:
 * snn = sum of n_i (n_i - 1) over the group's populations / (N (N - 1)) by the formula above, and
 * ge = n_perms.  beg >= end gives zero differences.  A window outside [0, n_rows] is not read: it gives
 * zero differences and the next pbg_check returns PBG_E_RANGE.  Everything is integers and order-fixed
 * doubles: two runs give the same bytes, and a window's result depends on key0 + beg, the rows and the
 * options only, not on its place in the list.  A NULL member of pbg_snn_out is skipped; with diff NULL and
 * groups asked for the matrix lives in a buffer of the context, which such calls share: keep them on one
 * stream.  n_groups = 0 is the difference matrix alone, valid for one population too.  Asynchronous; no workspace and no plan; the group
 * list is copied to the device once per content.  pbg_snn_chunks is the number of permutation chunks the
 * call's second kernel runs per (window, group) -- the host's choice, for tests and timing.  PBG_E_ARG for
 * a null ctx, rows, wins, opts or out, n_groups outside 0..PBG_SNN_MAX_GROUPS, n_perms outside
 * 0..PBG_SNN_MAX_PERMS, groups NULL with n_groups > 0, a group with fewer than two populations or with a
 * bit at or above n_pops, and (with groups) a context whose pop_n[i] is not the number of samples in
 * pop_mask[i]; n_win == 0 returns PBG_OK. */
#define PBG_SNN_MAX_GROUPS 4096
#define PBG_SNN_MAX_PERMS  65535
typedef struct { const uint64_t *groups;   /* HOST array [n_groups]: bit i = population i belongs to the group */
                 int32_t n_groups, n_perms; uint32_t seed, key0; } pbg_snn_opts;
typedef struct {            /* DEVICE arrays, caller-allocated, NULL = not wanted */
    int32_t *diff;          /* [n_win * n(n-1)/2]   */
    double  *snn;           /* [n_win * n_groups]   */
    int32_t *near;          /* [n_win * n_groups * 2] */
    int32_t *ge;            /* [n_win * n_groups]   */
} pbg_snn_out;
int pbg_window_snn(pbg_ctx *ctx, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                   const pbg_snn_opts *opts, const pbg_snn_out *out, void *stream);
int pbg_snn_chunks(uint32_t n_win, int32_t n_groups, int32_t n_perms);

/* Waits for `stream` and reports what the kernels flagged since the last check: PBG_OK;
 * PBG_E_BATCH when a pileup batch's block_off disagreed with its k[] (the affected blocks
 * were written as uncounted rows and never read past their key range); PBG_E_RANGE when the
 * statistics workspace (windows with more than 256 segregating sites, LD lists; up to 4 GiB)
 * ran out -- the windows that could not get a slice have unset outputs. */
int pbg_check(pbg_ctx *ctx, void *stream);

/* "product" for the shipped build; "bounds" for the PBG_BOUNDS debug build (key loads checked);
 * "experiment" for a timing variant built with experiment switches (tools/variant.sh) -- some of
 * which give wrong results, so nothing may ship or benchmark one as the product. */
const char *pbg_build_info(void);

/* ---- one subcommand end to end ------------------------------------------------------ */
enum { PBG_CMD_SNP = 0, PBG_CMD_HAPLO = 1, PBG_CMD_DIVERGE = 2, PBG_CMD_TREE = 3,
       PBG_CMD_NUCDIV = 4, PBG_CMD_LD = 5, PBG_CMD_SFS = 6 };   /* popbam_func_t (popbam.h:208) */

enum { PBG_LD_RMIN = 4 };   /* pbg_cmd.output of PBG_CMD_LD: bit 2 */
enum { PBG_HAPLO_NSL = 4 }; /* pbg_cmd.output of PBG_CMD_HAPLO: bit 2 */
enum { PBG_HAPLO_XPNSL = 8 }; /* pbg_cmd.output of PBG_CMD_HAPLO: bit 3 */
enum { PBG_NUCDIV_SNN = 1 };  /* pbg_cmd.output of PBG_CMD_NUCDIV: bit 0 = --snn, bits 1-16 PERMS, bits 17-30 SEED */
#define PBG_NUCDIV_SNN_PERMS(output) (((output) >> 1) & 0xFFFF)
#define PBG_NUCDIV_SNN_SEED(output)  (((output) >> 17) & 0x3FFF)

typedef struct {
    int32_t  cmd;          /* PBG_CMD_*                                                   */
    int32_t  output;       /* -o; sfs: bit 0 = --theta, bit 1 = --joint (a streamed run also runs
                              pbg_window_jsfs on the command's windows with outidx and appends,
                              per pair i < j, "fst[popI,popJ]:" (NA for NaN) and "jsfs[popI,popJ]:"
                              the pair's cells, comma-separated in cell order, after the
                              reference's columns and --theta's); bit 2 = --dstat (with three or
                              more populations a streamed run also runs pbg_window_dstat with
                              outidx over all triples (i, j, k), i < j, k not i or j, in
                              lexicographic order and appends, per triple, "D[popI,popJ,popK]:",
                              "fd[popI,popJ,popK]:", "fdM[popI,popJ,popK]:" (NA for NaN) and
                              "dsum[popI,popJ,popK]:" the six sums, comma-separated, after
                              --joint's columns; more than PBG_DSTAT_MAX_TRIPLES triples, i.e.
                              more than 21 populations: PBG_E_ARG); ld: bits 0-1 = -o (0, 1, 2),
                              PBG_LD_RMIN = --rmin (a streamed run also runs pbg_window_rmin on the
                              command's windows with min_freq and appends, per population,
                              "Rmin[pop]:" the count and "rint[pop]:" the chosen intervals as
                              left-right in 1-based contig positions, comma-separated (NA when the
                              count is 0), after the reference's columns and --decay's; they ignore
                              min_snps).  A bit of `output` and no new field: sizeof(pbg_cmd) stays,
                              so a program compiled against the header before it keeps running;
                              haplo: bits 0-1 = -o (0, 1, 2), PBG_HAPLO_NSL = --nsl, again a bit and no
                              new field (a streamed run also runs pbg_window_nsl on the command's
                              windows and appends, per population, "nsl[pop]:" one pos:m:value:c per
                              variable site, comma-separated -- pos the 1-based contig position,
                              value the unstandardised nSL as %.5f or NA, c = cens[0] + cens[1] -- or
                              NA when there is none, after the reference's columns and hfs's; they
                              ignore min_sites); PBG_HAPLO_XPNSL = --xpnsl, a bit likewise (a streamed
                              run also runs pbg_window_xpnsl and appends, per population pair i < j,
                              "xpnsl[popI,popJ]:" one pos:mI:mJ:value:c per pooled site -- value the
                              unstandardised XP-nSL as %.5f or NA, c = cens[0] + cens[1] -- or NA when
                              there is none, after --nsl's columns; nothing with fewer than two
                              populations; they ignore min_sites); nucdiv (which has no -o):
                              PBG_NUCDIV_SNN = --snn, with PERMS in bits 1-16 and SEED in bits 17-30
                              (PBG_NUCDIV_SNN_PERMS, PBG_NUCDIV_SNN_SEED), again no new field: with two
                              or more populations a streamed run also runs pbg_window_snn on the
                              command's windows with key0 = the contig position of row 0 -- the groups
                              are all populations together (first, and only with three or more), then
                              every pair i < j in lexicographic order -- and appends, per group,
                              "snn[NAMES]:" and "psnn[NAMES]:" as %.5f, NAMES being popI,popJ or *,
                              psnn = (ge + 1) / (PERMS + 1); both are NA for a window without a
                              segregating site, psnn also when PERMS is 0; -k does not blank them   */
    int32_t  min_sites;    /* -k                                                          */
    int32_t  min_snps;     /* ld -n                                                       */
    int32_t  min_freq;     /* ld 1 / 2 (-e)                                               */
    int32_t  outidx;       /* -p sample index                                             */
    int32_t  jc;           /* diverge / tree -d jc                                        */
    int32_t  windowed;     /* -w given                                                    */
    int64_t  win_size;     /* bases                                                       */
    int32_t  beg, end;     /* parsed region [beg, end) in contig coordinates              */
    const char *chr_name;
    const char *const *sample_names;
    const char *const *pop_names;
    const char *refid;     /* tree: taxon name of the reference (get_refid, pop_utils.cpp:463-498:
                              the header's first AS: tag value)                              */
    int32_t  ms_windows;   /* snp -o 2 header (print_ms, pop_snp.cpp:114-115, printed before the
                              first window): 0 = this call's window count; > 0 = print it with
                              this total (a block of a longer run that starts the run);
                              < 0 = no header (a later block of a longer run)                */
    int32_t  decay_bin, decay_bins;   /* ld -o 0 --decay=BIN,NBINS (0 = off): a streamed run also
                              bins r^2 by distance (pbg_window_ld_decay on the command's windows) and
                              appends, per population, "decay[pop]:" the bins' mean r^2 (NA for an
                              empty bin) and "pairs[pop]:" their pair counts, comma-separated, after
                              the reference's columns; they ignore min_snps                      */
    int32_t  hfs;          /* haplo --hfs (any -o; 0 = off): a streamed run also runs pbg_window_hfs on
                              the command's windows and appends, per population, "H1[pop]:",
                              "H12[pop]:", "H123[pop]:", "H2H1[pop]:", "Hd[pop]:" (NA for NaN) and
                              "hfs[pop]:" the K class sizes, comma-separated, after the reference's
                              columns; they ignore min_sites                                      */
} pbg_cmd;

/* Runs `popbam <cmd>` over a HOST pileup batch that covers contig positions
 * [pileup->pos0, pileup->pos0 + n_sites) (host pointers; block_off may be NULL and is then
 * derived from k[]): one stream (pbg_stream_*, below) over the 64-position blocks the
 * command's windows touch.  Writes the reference's stdout (TSV) into out (NUL-terminated).
 * Returns the text length, or PBG_E_RANGE with *needed set when cap is too small; the text
 * is then kept by the context and pbg_take_text() copies it without running again.       */
long pbg_run(pbg_ctx *ctx, const pbg_cmd *cmd, const pbg_pileup *host_pileup, char *out,
             size_t cap, size_t *needed);
long pbg_take_text(pbg_ctx *ctx, char *out, size_t cap);

/* print_<stat> for windows whose results were copied to the HOST: `host_out` holds host
 * arrays laid out as pbg_window_out, `wbeg`/`wend` the contig coordinates the reference
 * prints (+1 applied here).  Same return convention as pbg_run.  It takes no decay arrays and
 * prints the reference's columns only, whatever the command's decay_bin says; no joint-spectrum
 * arrays and no D-statistic arrays either, so sfs output bits 1 (--joint) and 2 (--dstat) add
 * nothing here; no haplotype-spectrum arrays, so haplo's hfs adds nothing here; no Rmin arrays,
 * so ld's PBG_LD_RMIN adds nothing here; no nSL arrays, so haplo's PBG_HAPLO_NSL adds nothing here;
 * no XP-nSL arrays, so haplo's PBG_HAPLO_XPNSL adds nothing here; no Snn arrays, so nucdiv's
 * PBG_NUCDIV_SNN adds nothing here. */
long pbg_format(const pbg_ctx *ctx, const pbg_cmd *cmd, const pbg_window_out *host_out, uint32_t n_win,
                const int32_t *wbeg, const int32_t *wend, char *out, size_t cap, size_t *needed);

/* ---- streamed runs over HOST batches ------------------------------------------------- */
/* The host side of the pileup callback produces a region's key batch position by position; a
 * stream takes it in pieces, in position order, while the walk goes on (the reference instead
 * re-fetches and re-piles every window, pop_nucdiv.cpp:57-125, and calls each position inside
 * the callback).  Each pushed piece is copied to the device in chunks that alternate between
 * two device slots (the copy of chunk i+1 runs under the call of chunk i) and called into the
 * region's rows; pbg_stream_finish then runs every command's windows (main_<cmd>'s window loop)
 * over those rows and prints their TSV.  Slots, pinned staging, the rows buffer and the window
 * lists (with their statistics plans) belong to the context and serve the next stream: a steady
 * state of streams allocates nothing.  One open stream per context; pbg_run is one stream of
 * one command over one piece.
 *   cmds         the commands to print (all over the same region; the pointers inside them --
 *                names -- must stay valid until pbg_stream_finish); snp -o 0 keeps consensus words
 *   pos0,n_sites the region [pos0, pos0 + n_sites) of contig positions the pieces cover
 *   chunk_sites  positions per device slot (0: about 256 MB of pileup per slot)
 * A piece (host pointers, block_off may be NULL: derived from k[]) starts where the previous
 * one ended and holds a multiple of 64 positions unless it is the last.  Pageable buffers are
 * copied before pbg_stream_push returns; pinned ones (hipHostMalloc / hipHostRegister) are read
 * by DMA asynchronously and must stay unchanged until pbg_stream_finish.                     */
typedef struct pbg_stream pbg_stream;
typedef struct {
    uint64_t h2d_bytes;      /* bytes copied host -> device                                   */
    uint32_t pieces, chunks; /* pushes; device chunks                                          */
    uint32_t pinned_chunks;  /* chunks copied straight from pinned caller buffers              */
    uint32_t _pad;
    double   ms_stage;       /* host: pageable pieces -> pinned staging (threaded memcpy)      */
    double   ms_wait;        /* host: waiting for a slot's previous copy                       */
    double   ms_h2d;         /* device: the chunks' H2D copies (events on the copy stream)     */
    double   ms_call;        /* device: pbg_call_sites per chunk (events on the compute stream) */
    double   ms_finish;      /* host: pbg_stream_finish (wait, statistics, D2H, printing)      */
} pbg_stream_prof;
int  pbg_stream_open(pbg_ctx *ctx, const pbg_cmd *cmds, uint32_t n_cmd, int32_t pos0, uint32_t n_sites,
                     uint32_t chunk_sites, pbg_stream **st);
int  pbg_stream_push(pbg_stream *st, const pbg_pileup *host_piece);
/* The same for a COMPACT piece (rows-only streams: not snp -o 0; max_depth <= 33025): a task
 * (position, sample) whose rmsq[] has bit 31 set is reference-only -- the position is called back
 * (ref bit 7 clear), its reference byte is an upper-case A/C/G/T, it has 1..32 keys and every key
 * shows that base -- and its keys are left out of keys[]: block_off counts the keys present, k[]
 * keeps the task's key count and rmsq[] bits 0..30 its sum of mapQ^2 (qfilter).  The scan settles
 * such a task from k and rmsq alone (it does the same for the full piece's reference-only tasks),
 * so the rows equal the full piece's; the other tasks are exactly as in pbg_stream_push.  About
 * 92 % of the keys of a depth-10 panel belong to reference-only tasks, so the piece crosses PCIe
 * in about a quarter of the bytes.  A flag on a task that cannot be reference-only is reported by
 * pbg_stream_finish (PBG_E_BATCH).  Replaces nothing in the reference: call_base's per-read loop
 * (popbam.cpp:266-287) already walks every key of the task, where the test costs a compare. */
int  pbg_stream_push_compact(pbg_stream *st, const pbg_pileup *host_piece);
int  pbg_stream_finish(pbg_stream *st);   /* waits, checks (PBG_E_BATCH ...), prints every command */
/* command i's text (NUL-terminated); returns its length or PBG_E_RANGE with *needed set       */
long pbg_stream_text(pbg_stream *st, uint32_t i, char *out, size_t cap, size_t *needed);
/* copies the region's packed rows (n_sites * pbg_row_bytes() bytes) into dst, host or device
 * memory (the statistics' input: lets a caller check a streamed run against a resident one)   */
int  pbg_stream_rows(const pbg_stream *st, void *dst, size_t cap);
int  pbg_stream_profile(const pbg_stream *st, pbg_stream_prof *prof);
/* the message of the stream's error (its context's last error; "" when it has none): for a
 * caller that holds the stream but not the context, e.g. a pileup callback                 */
const char *pbg_stream_error(const pbg_stream *st);
void pbg_stream_close(pbg_stream *st);

/* ---- profiling ---------------------------------------------------------------------- */
/* With timing on, every pbg_call_sites records a pair of HIP events on its stream around its
 * dominant kernel (the scan kernel of the rows-only pipeline, the block kernel when
 * consensus words are requested) and one pair around the whole call; pbg_kernel_time waits
 * for the recorded events and returns the summed elapsed milliseconds of each and the number
 * of calls timed.  Turning timing on (again) restarts the count.  No reference counterpart
 * (the reference has no timers).                                                  */
int pbg_set_kernel_timing(pbg_ctx *ctx, int on);
int pbg_kernel_time(pbg_ctx *ctx, double *ms_total, uint32_t *launches);
int pbg_call_time(pbg_ctx *ctx, double *ms_total, uint32_t *launches);

/* ---- synthetic workload (benchmark) ------------------------------------------------- */
/* Counter-based pileup generator (splitmix64 keyed on (seed, contig, position);
 * depth ~ Binomial(2 * mean_depth, 1/2), baseQ 20..40, mapQ 60, ~0.8 % error bases, theta
 * ~1.2 %), written straight into device memory in the pbg_pileup layout with the context's
 * filters applied (the keys the host side of the callback would have built).  Positions
 * [pos0, pos0 + n_sites) of `contig`; block_off is relative to this batch.  A task's reads
 * are a window of a per-seed table of 2^20 random read templates (built on the first call
 * with a seed, which then synchronises `stream` once).  ref / k / rmsq / keys must be 16-byte
 * aligned.                                                                                  */
typedef struct {
    uint64_t seed;
    int32_t  contig;
    int32_t  mean_depth;   /* 1..32                                                       */
    int64_t  pos0;
    uint32_t n_sites;
} pbg_synth_spec;

/* Upper bound on the keys of a batch (n_sites * n * 2 * mean_depth): a keys[] buffer this
 * large lets pbg_synth_pileup run without any host synchronisation.                       */
uint64_t pbg_synth_max_keys(const pbg_ctx *ctx, const pbg_synth_spec *spec);
/* Fills ref / k / rmsq / block_off / keys (device).  keys_cap = capacity of keys[] in keys;
 * a batch that needs more fails at the next pbg_check (PBG_E_BATCH) with no write past it.
 * keys = NULL (keys_cap 0) fills everything but the keys (a counting pass).  n_keys (host,
 * may be NULL) receives the key count and makes the call synchronous.                     */
int pbg_synth_pileup(pbg_ctx *ctx, const pbg_synth_spec *spec, uint8_t *ref, void *k, uint32_t *rmsq,
                     uint64_t *block_off, uint16_t *keys, uint64_t keys_cap, uint64_t *n_keys, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* POPBAM_GPU_H */
