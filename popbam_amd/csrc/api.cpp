// api.cpp -- the C-ABI of include/popbam_gpu.h: context, resident-batch launches
// (pbg_call_sites / pbg_window_stats / pbg_check), the synthetic generator and pbg_format.
// Streamed runs over host batches (pbg_stream_*, pbg_run) are in stream.cpp.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "pbg_ctx.h"


namespace {

thread_local std::string g_create_error;

int fail(pbg_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    else g_create_error = msg;
    return code;
}

}  // namespace

int pbg::ctx_fail(pbg_ctx *c, int code, const std::string &msg) { return fail(c, code, msg); }

namespace {

#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess)                                                                      \
            return fail((ctx), PBG_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
    } while (0)

// rms of call_base (popbam.cpp:292) for k keys with sum mapQ^2 = rmsq: the reference's float
// division, sqrtf and (unsigned long long)(x + 0.499)
uint32_t rms_of(uint32_t rmsq, int k) {
    const float f = (float)rmsq / (float)k;
    return (uint32_t)((double)std::sqrt(f) + 0.499);
}
// smallest sum mapQ^2 (mapQ <= 255) whose rms passes qfilter with k keys, or ~0 when none does
uint32_t rms_threshold(int k, int min_rmsQ, int min_depth, int max_depth) {
    if (k < 1 || k < min_depth || k > max_depth) return 0xFFFFFFFFu;
    uint32_t lo = 0, hi = (uint32_t)k * 65025u;   // rms is monotone in rmsq
    if ((int)rms_of(hi, k) < min_rmsQ) return 0xFFFFFFFFu;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((int)rms_of(mid, k) >= min_rmsQ) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

int row_bytes_for(int n) { return n <= 14 ? 2 : n <= 30 ? 4 : n <= 62 ? 8 : 16; }

template <class T>
hipError_t upload(T **dst, const std::vector<T> &v) {
    hipError_t e = hipMalloc((void **)dst, std::max<size_t>(1, v.size()) * sizeof(T));
    if (e != hipSuccess) return e;
    if (v.empty()) return hipSuccess;
    return hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}


}  // namespace

namespace {
// off[p] of every pair i < j in lexicographic order, and off[n_pairs] = C (include/popbam_gpu.h)
std::vector<int32_t> jsfs_offsets(const pbg::DevParams &dp) {
    std::vector<int32_t> off;
    int32_t at = 0;
    for (int i = 0; i < dp.npops; ++i)
        for (int j = i + 1; j < dp.npops; ++j) {
            off.push_back(at);
            at += (dp.pop_n[i] + 1) * (dp.pop_n[j] + 1);
        }
    off.push_back(at);
    return off;
}

// argument checks shared by the side tables' calls; `what` is the call's prefix in the message
// ("jsfs", "dstat", "hfs").  The kernels count within pop_mask and subtract from or divide by pop_n.
int check_pop_sizes(pbg_ctx *c, const char *what) {
    for (int i = 0; i < c->dp.npops; ++i)
        if (__builtin_popcountll(c->dp.pop_mask[i]) + __builtin_popcountll(c->dp.pop_mask_hi[i]) != c->dp.pop_n[i])
            return fail(c, PBG_E_ARG, std::string(what) + ": pop_n must be the number of samples in pop_mask");
    return PBG_OK;
}
// the outgroup's sample index to hand the kernel (-1: the context does not flip)
int check_outidx(pbg_ctx *c, const char *what, int32_t outidx, int32_t *flip_idx) {
    *flip_idx = -1;
    if (!(c->dp.flag & PBG_F_OUTGROUP)) return PBG_OK;
    if (outidx < 0 || outidx >= c->dp.n) return fail(c, PBG_E_ARG, std::string(what) + ": outidx must be a sample index");
    *flip_idx = outidx;
    return PBG_OK;
}

// a device window list, copied to the host for the caller to validate (this synchronises: the
// callers cache what they validated)
int fetch_windows(pbg_ctx *c, const pbg_window *wins, uint32_t n_win, hipStream_t stream, std::vector<pbg_window> &hw) {
    hw.resize(n_win);
    HIPCHK(c, hipMemcpyAsync(hw.data(), wins, n_win * sizeof(pbg_window), hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    return PBG_OK;
}
// The statistics workspace of pbg_window_stats and pbg_window_ld_decay: a pool the windows take
// slices of on the device, scratch within a call (calls on one stream run in order).  `worst` is the
// call's worst case in u64 words; the pool only ever grows, so either call's cached plans stay valid.
constexpr uint64_t kPoolMax = 512ull << 20;   // words (4 GiB)
int size_pool(pbg_ctx *c, uint64_t worst) {
    return pbg::grow(c, c->ws, std::max<uint64_t>(1024, std::min(worst, kPoolMax)) * 8);
}

// pbg_kernel_time / pbg_call_time: the summed time of the event pairs used since timing was set
int event_time(pbg_ctx *c, std::vector<std::pair<hipEvent_t, hipEvent_t>> pbg_ctx::*pairs, double *ms_total,
               uint32_t *launches) {
    if (!c || !ms_total || !launches) return fail(c, PBG_E_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    const auto &ev = c->*pairs;
    double tot = 0.0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        HIPCHK(c, hipEventSynchronize(ev[i].second));
        float ms = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev[i].first, ev[i].second));
        tot += ms;
    }
    *ms_total = tot;
    *launches = (uint32_t)c->ev_used;
    return PBG_OK;
}

// pbg_window_nsl and pbg_window_xpnsl: the shared checks (messages prefixed by `name`), then the launch.
// A call whose chains need at least min_pops populations writes nothing below that.
template <class Opts, class Out, class Launch>
int window_tract(pbg_ctx *c, const char *name, int min_pops, const void *rows, uint32_t n_rows, const pbg_window *wins,
                 uint32_t n_win, const Opts *o, const Out *out, void *stream, Launch launch) {
    const std::string nm = name;
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    if (o->max_sites < 0) return fail(c, PBG_E_ARG, nm + ": max_sites must not be negative");
    if ((out->row || out->m || out->sl || out->cens) && o->max_sites == 0)
        return fail(c, PBG_E_ARG, nm + ": row, m, sl and cens need max_sites of at least 1");
    if ((out->sl || out->cens) && !out->row) return fail(c, PBG_E_ARG, nm + ": sl and cens need row");
    if (int rc = check_pop_sizes(c, name)) return rc;   // the pairs come from pop_n, the samples from pop_mask
    if (n_win == 0 || c->dp.npops < min_pops) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    pbg::TractArgs A{};
    A.wins = wins;
    A.err = c->d_err;
    A.max_sites = o->max_sites;
    A.n_var = out->n_var;
    A.row = out->row;
    A.m = out->m;
    A.sl = out->sl;
    A.cens = out->cens;
    HIPCHK(c, launch(c->row_bytes, c->dp, rows, n_rows, n_win, A, (hipStream_t)stream));
    return PBG_OK;
}
}  // namespace

namespace pbg {
extern const int kBuildKind_call, kBuildKind_stats, kBuildKind_decay, kBuildKind_jsfs, kBuildKind_dstat, kBuildKind_hfs,
    kBuildKind_rmin, kBuildKind_nsl, kBuildKind_xpnsl, kBuildKind_snn;
}

namespace {
// errmod_tables.bin beside this library (written by `make`, pbg_host.h)
std::string tables_path() {
    Dl_info info;
    if (!dladdr((void *)&pbg_create, &info) || !info.dli_fname) return std::string();
    std::string p = info.dli_fname;
    const size_t sl = p.rfind('/');
    return (sl == std::string::npos ? std::string(".") : p.substr(0, sl)) + "/errmod_tables.bin";
}
}  // namespace

extern "C" {

int pbg_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char *pbg_last_error(const pbg_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int pbg_row_bytes(const pbg_ctx *ctx) { return ctx ? ctx->row_bytes : 0; }
int pbg_k_bytes(const pbg_ctx *ctx) { return ctx ? (ctx->dp.k16 ? 2 : 1) : 0; }
int pbg_sfs_stride(const pbg_ctx *ctx) { return ctx ? ctx->dp.sfs_stride : 0; }
int pbg_hfs_stride(const pbg_ctx *ctx) { return ctx ? ctx->dp.pop_nmax : 0; }

int pbg_create(pbg_ctx **out, int device, const pbg_params *p) {
    if (!out || !p) return fail(nullptr, PBG_E_ARG, "null argument");
    *out = nullptr;
    if (p->n_samples < 1 || p->n_samples > PBG_MAX_SAMPLES)
        return fail(nullptr, PBG_E_ARG, "n_samples must be in [1, 126]");
    if (p->n_pops < 1 || p->n_pops > PBG_MAX_POPS) return fail(nullptr, PBG_E_ARG, "n_pops must be in [1, 64]");
    if (p->max_depth < 0 || p->max_depth > 65535) return fail(nullptr, PBG_E_ARG, "max_depth must be in [0, 65535]");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, PBG_E_NODEV, "no HIP device visible (libpopbam_gpu has no CPU path)");
    if (device < 0 || device >= ndev) return fail(nullptr, PBG_E_NODEV, "device index out of range");
    pbg_ctx *c = new pbg_ctx();
    c->device = device;
    c->params = *p;
    c->row_bytes = row_bytes_for(p->n_samples);
    pbg::DevParams &d = c->dp;
    d.n = p->n_samples;
    d.npops = p->n_pops;
    for (int i = 0; i < PBG_MAX_POPS; ++i) {
        d.pop_mask[i] = i < p->n_pops ? p->pop_mask[i] : 0;
        d.pop_mask_hi[i] = i < p->n_pops && p->n_samples > 64 ? p->pop_mask_hi[i] : 0;
        d.pop_n[i] = i < p->n_pops ? p->pop_n[i] : 0;
    }
    d.min_depth = p->min_depth;
    d.max_depth = p->max_depth;
    d.min_rmsQ = p->min_rmsQ;
    d.min_snpQ = p->min_snpQ;
    d.min_mapQ = p->min_mapQ & 0xff;
    d.min_baseQ = p->min_baseQ & 0xff;
    d.flag = p->flag;
    d.k16 = p->max_depth > 255 ? 1 : 0;
    // population of each sample: assign_pops gives every sample one population (popbam.cpp:145-171)
    for (int v = 0; v < PBG_MAX_SAMPLES; ++v) d.sample_pop[v] = -1;
    for (int i = 0; i < p->n_pops; ++i)
        for (int v = 0; v < p->n_samples; ++v)
            if (((v < 64 ? p->pop_mask[i] >> v : d.pop_mask_hi[i] >> (v - 64)) & 1)) {
                if (d.sample_pop[v] >= 0) {
                    delete c;
                    return fail(nullptr, PBG_E_ARG, "population masks overlap");
                }
                d.sample_pop[v] = (int8_t)i;
            }
    {   // samples grouped by population (window statistics: per-population-pair loops)
        int at = 0;
        for (int i = 0; i < p->n_pops; ++i) {
            d.pop_start[i] = (int16_t)at;
            for (int v = 0; v < p->n_samples; ++v)
                if (d.sample_pop[v] == i) d.pop_member[at++] = (uint8_t)v;
        }
        for (int i = p->n_pops; i <= PBG_MAX_POPS; ++i) d.pop_start[i] = (int16_t)at;
        d.pop_nmax = 0;
        d.pops_ordered = 1;
        int last = -1;   // largest member id of the populations so far
        for (int i = 0; i < p->n_pops; ++i) {
            const int a0 = d.pop_start[i], a1 = d.pop_start[i + 1];
            d.pop_nmax = std::max(d.pop_nmax, a1 - a0);
            if (a1 > a0) {
                if (d.pop_member[a0] < last) d.pops_ordered = 0;
                last = d.pop_member[a1 - 1];
            }
        }
    }
    for (int k = 0; k <= PBG_FAST_MAX; ++k) d.rms_thr[k] = rms_threshold(k, p->min_rmsQ, p->min_depth, p->max_depth);
    d.rmsq_thr[0] = p->min_rmsQ <= 0 ? 0u : 0xFFFFFFFFu;
    for (int k = 1; k <= 16; ++k) d.rmsq_thr[k] = rms_threshold(k, p->min_rmsQ, 1, 1 << 30);
    d.sfs_stride = 1;
    for (int i = 0; i < p->n_pops; ++i) d.sfs_stride = std::max(d.sfs_stride, p->pop_n[i] + 1);
    auto bad = [&](hipError_t e, const char *what) {
        std::string m = std::string(what) + ": " + hipGetErrorString(e);
        pbg_destroy(c);
        return fail(nullptr, PBG_E_HIP, m);
    };
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return bad(e, "hipSetDevice");
    if ((e = hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device)) != hipSuccess)
        return bad(e, "hipDeviceGetAttribute");
    if (c->n_cu < 1) c->n_cu = 1;
    std::vector<double> fk, beta, lhet;
    if (!pbg::load_errmod_tables(tables_path().c_str(), fk, beta, lhet)) pbg::build_errmod_tables(fk, beta, lhet);
    // the scan's reference-only shortcut needs every beta[q][n][c < n] > 0 (q >= 4, n <= PBG_FAST_MAX)
    for (int q = 4; q < 64; ++q)
        for (int nn = 1; nn <= PBG_FAST_MAX; ++nn)
            for (int cc = 0; cc < nn; ++cc)
                if (!(beta[q << 16 | nn << 8 | cc] > 0.0)) {
                    pbg_destroy(c);
                    return fail(nullptr, PBG_E_ARG, "errmod beta table has a non-positive entry");
                }
    if ((e = upload(&c->d_fk, fk)) != hipSuccess) return bad(e, "upload fk");
    if ((e = upload(&c->d_beta, beta)) != hipSuccess) return bad(e, "upload beta");
    if ((e = upload(&c->d_lhet, lhet)) != hipSuccess) return bad(e, "upload lhet");
    {
        std::vector<double> fbeta(pbg::kFbetaSize, 0.0);
        for (uint32_t q = 0; q < 64; ++q)
            for (uint32_t nn = 0; nn < (uint32_t)pbg::kFbetaN; ++nn)
                for (uint32_t cc = 0; cc < 16; ++cc)
                    for (uint32_t w = 0; w < 16; ++w)
                        // q = 0 stays +0.0 (beta's q = 0 plane is never filled, pop_utils.cpp:230):
                        // the register path relies on it for its zero padding words
                        fbeta[pbg::fbeta_index(q, nn, cc, w)] = q ? fk[w] * beta[q << 16 | nn << 8 | cc] : 0.0;
        if ((e = upload(&c->d_fbeta, fbeta)) != hipSuccess) return bad(e, "upload fbeta");
        std::vector<double> lb(pbg::kLbSize, 0.0);
        for (int m = 1; m <= 16; ++m) lb[m] = lb[m - 1] + fk[m - 1];
        for (int d = 3; d <= 16; ++d) {
            double run = 1e300;   // suffix minimum over q' >= q
            for (int q = 63; q >= 4; --q) {
                for (int cc = 0; cc <= d - 2; ++cc) run = std::min(run, beta[q << 16 | d << 8 | cc]);
                lb[17 + (q - 4) * 17 + d] = run;
            }
        }
        if ((e = upload(&c->d_lb, lb)) != hipSuccess) return bad(e, "upload lb");
        std::vector<double> oe(pbg::kOeSize, 0.0);
        for (int q = 4; q < 64; ++q)
            for (int d = 0; d <= 16; ++d) oe[(q - 4) * 17 + d] = beta[q << 16 | d << 8];
        for (int nn = 0; nn <= 16; ++nn)
            for (int kk = 0; kk <= 16; ++kk) oe[60 * 17 + nn * 17 + kk] = lhet[nn << 8 | kk];
        if ((e = upload(&c->d_oe, oe)) != hipSuccess) return bad(e, "upload one-error tables");
        {   // call_scan_kernel's LDS image of the same tables (pbg_common.h ScanTab)
            pbg::ScanTab st{};
            for (int q = 4; q < 64; ++q)
                for (int dd = 3; dd <= 16; ++dd) {
                    const volatile double pe = fk[0] * beta[q << 16 | dd << 8];   // one_error_ref's product
                    st.fpe[(q - 4) * 14 + dd - 3] = (float)pe;
                }
            for (int lev = 0; lev < 15; ++lev)
                for (int dd = 3; dd <= 16; ++dd) {
                    const double b = lb[17 + (4 * lev) * 17 + dd];   // q = 4 + 4 lev: a bound for the level
                    float f = (float)b;
                    if ((double)f > b) f = std::nextafter(f, 0.0f);   // rounded down
                    st.lq[lev * 14 + dd - 3] = f;
                }
            for (int dd = 3; dd <= 16; ++dd) {
                const int idx[4][2] = {{dd, dd - 1}, {dd, 1}, {dd - 1, 0}, {dd - 1, dd - 1}};
                for (int i = 0; i < 4; ++i) {
                    const volatile double h = -4.343 * lhet[idx[i][0] << 8 | idx[i][1]];
                    st.lh[(dd - 3) * 4 + i] = h;
                }
            }
            for (int m = 0; m <= 16; ++m) st.pre[m] = lb[m];
            if ((e = hipMalloc(&c->d_scantab, sizeof(st))) != hipSuccess) return bad(e, "hipMalloc scan tables");
            if ((e = hipMemcpy(c->d_scantab, &st, sizeof(st), hipMemcpyHostToDevice)) != hipSuccess)
                return bad(e, "upload scan tables");
        }
        std::vector<double> bu(60 * 17, 0.0);   // min over q' >= q, c <= d - 1 of beta[q'][d][c]
        for (int dd = 1; dd <= 16; ++dd) {
            double run = 1e300;
            for (int q = 63; q >= 4; --q) {
                for (int cc = 0; cc <= dd - 1; ++cc) run = std::min(run, beta[q << 16 | dd << 8 | cc]);
                bu[(q - 4) * 17 + dd] = run;
            }
        }
        // uniform tasks: het values and the strand-free bound per (d, m class, q); since fk
        // decreases, fk_prefix[m0] + fk_prefix[m1] >= fk_prefix[m0 + m1], so fk_prefix[d] is a
        // lower bound of the per-strand sum whatever the strands
        bool fk_dec = true;   // fk[n] = (1 - depcorr)^n (1 - eta) + eta (pop_utils.cpp:219) decreases
        for (int w = 1; w < 16; ++w) fk_dec = fk_dec && fk[w] <= fk[w - 1];
        for (int i = 0; i < 17 * 3; ++i) d.uni[i] = 255u;
        for (int dd = 1; dd <= 16; ++dd) {
            float h[2];
            for (int t = 0; t < 2; ++t) {   // het m/x with c_hi = 0 / d: (float)(-4.343 lhet), clamped
                const float v = (float)(-4.343 * lhet[dd << 8 | (t ? dd : 0)]);
                h[t] = v < 0.0f ? 0.0f : v;
            }
            const float hm[3] = {h[0], h[1], std::min(h[0], h[1])};
            for (int cls = 0; cls < 3; ++cls) {
                uint32_t qthr = 255u;   // the bound grows with q_min (suffix minimum): first passing q
                for (int q = 63; q >= 4; --q) {
                    const double lbv = lb[dd] * bu[(q - 4) * 17 + dd];
                    if (fk_dec && hm[cls] > 0.0f && lbv * (1.0 - 1e-9) > (double)hm[cls] * (1.0 + 1e-6) + 1e-3) qthr = (uint32_t)q;
                    else break;
                }
                const uint32_t snpq = (uint32_t)(uint64_t)((double)hm[cls] + 0.499) & 0xFFFFu;
                d.uni[dd * 3 + cls] = qthr | snpq << 8;
            }
        }
    }
    // Tajima constants are indexed by population size and built for n = sm->n (pop_sfs.cpp:53-56)
    std::vector<double> a1, a2, e1, e2;
    pbg::build_sfs_constants(p->n_samples, a1, a2, e1, e2);
    const size_t L = a2.size();
    std::vector<double> sfs(4 * L, 0.0);
    std::copy(a1.begin(), a1.end(), sfs.begin());
    std::copy(a2.begin(), a2.end(), sfs.begin() + L);
    std::copy(e1.begin(), e1.end(), sfs.begin() + 2 * L);
    std::copy(e2.begin(), e2.end(), sfs.begin() + 3 * L);
    if ((e = upload(&c->d_sfs, sfs)) != hipSuccess) return bad(e, "upload sfs constants");
    std::vector<double> r2all;
    for (int i = 0; i < p->n_pops; ++i) {
        std::vector<double> t;
        pbg::build_r2_table(std::max(1, p->pop_n[i]), t);
        c->dt.r2_off[i] = (int32_t)r2all.size();
        r2all.insert(r2all.end(), t.begin(), t.end());
    }
    if ((e = upload(&c->d_r2, r2all)) != hipSuccess) return bad(e, "upload r2 tables");
    if ((e = hipMalloc(&c->d_err, sizeof(int))) != hipSuccess) return bad(e, "hipMalloc err");
    if ((e = hipMemset(c->d_err, 0, sizeof(int))) != hipSuccess) return bad(e, "hipMemset err");
    c->dt.fk = c->d_fk;
    c->dt.beta = c->d_beta;
    c->dt.lhet = c->d_lhet;
    c->dt.fbeta = c->d_fbeta;
    c->dt.lb = c->d_lb;
    c->dt.oe = c->d_oe;
    c->dt.scantab = reinterpret_cast<const uint4 *>(c->d_scantab);
    c->dt.a1 = c->d_sfs;
    c->dt.a2 = c->d_sfs + L;
    c->dt.e1 = c->d_sfs + 2 * L;
    c->dt.e2 = c->d_sfs + 3 * L;
    c->dt.r2 = c->d_r2;
    *out = c;
    return PBG_OK;
}

void pbg_destroy(pbg_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    pbg::stream_bufs_free(c);
    for (void *p : {(void *)c->d_fk, (void *)c->d_beta, (void *)c->d_lhet, (void *)c->d_sfs, (void *)c->d_r2,
                    (void *)c->d_fbeta, (void *)c->d_lb, (void *)c->d_oe, c->d_scantab, (void *)c->d_err,
                    (void *)c->deep.sites, (void *)c->deep.tasks, (void *)c->deep.info, (void *)c->deep.count,
                    (void *)c->deep.blk_cnt, (void *)c->deep.raw, (void *)c->deep.pend,
                    (void *)c->d_decay_used, (void *)c->jsfs.d_pairs, (void *)c->jsfs.d_groups})
        if (p) (void)hipFree(p);
    for (pbg::DevBuf *b : {&c->ws, &c->wsoff, &c->zns, &c->segcnt, &c->synth, &c->snn_diff})
        if (b->d) (void)hipFree(b->d);
    for (auto &t : c->tmpl) (void)hipFree(t.second);
    for (auto &l : c->dstat_lists)
        if (l.d) (void)hipFree(l.d);
    for (auto &l : c->snn_lists)
        if (l.d) (void)hipFree(l.d);
    for (auto *v : {&c->ev, &c->evc})
        for (auto &e : *v) {
            (void)hipEventDestroy(e.first);
            (void)hipEventDestroy(e.second);
        }
    delete c;
}

int pbg_call_sites(pbg_ctx *c, const pbg_pileup *pl, void *rows, uint64_t *cb, void *stream) {
    if (!c || !pl || !rows) return fail(c, PBG_E_ARG, "null argument");
    if (pl->n_sites == 0) return PBG_OK;
    if (!pl->ref || !pl->k || !pl->rmsq || !pl->block_off || !pl->keys) return fail(c, PBG_E_ARG, "null pileup array");
    if (((uintptr_t)pl->keys | (uintptr_t)pl->k | (uintptr_t)pl->rmsq | (uintptr_t)rows) & 15)
        return fail(c, PBG_E_ARG, "keys / k / rmsq / rows must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t nblk = (pl->n_sites + pbg::kSiteBlock - 1) / pbg::kSiteBlock;
    const int64_t hint = c->cap_hint_keys;
    c->cap_hint_keys = -1;
    if (cb && (hint >= 0 || c->cap_key != (const void *)pl->block_off || c->cap_sites != pl->n_sites)) {
        // LDS staging capacity of the consensus-word kernel: the mean round plus six standard
        // deviations (Poisson-like), bounded by what one CU can give a workgroup; rounds above
        // it read HBM directly.  The batch's keys are block_off[nblk] - block_off[0] (offsets may
        // be absolute, include/popbam_gpu.h); a streamed chunk passes its count from the host
        uint64_t total = 0;
        if (hint >= 0) {
            total = (uint64_t)hint;
        } else {
            uint64_t ends[2] = {0, 0};
            HIPCHK(c, hipMemcpyAsync(&ends[0], pl->block_off, sizeof(uint64_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
            HIPCHK(c, hipMemcpyAsync(&ends[1], pl->block_off + nblk, sizeof(uint64_t), hipMemcpyDeviceToHost,
                                     (hipStream_t)stream));
            HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
            total = ends[1] >= ends[0] ? ends[1] - ends[0] : 0;
        }
        // keys staged per round = keys of kBlockThreads consecutive (position, sample) tasks
        const double mean = (double)total / ((double)pl->n_sites * c->dp.n) * pbg::kBlockThreads;
        uint32_t cap = (uint32_t)(mean + 6.0 * std::sqrt(mean) + 64.0);
        cap = (cap + 63) & ~63u;
        const uint32_t max_cap = (uint32_t)((48 * 1024 - pbg::call_sites_lds_bytes(c->dp.n, 0)) / 4);
        c->cap_val = std::min(std::max(cap, 256u), max_cap);
        c->cap_key = hint >= 0 ? nullptr : pl->block_off;   // a hinted chunk's slot pointer repeats
        c->cap_sites = pl->n_sites;
    }
    const uint32_t cap = c->cap_val;
    // queues: positions (worst case all), parked info bytes (n per position), per-block queue
    // regions of 3/16 of the block's tasks (+32) for the rows-only pipeline (segregating
    // positions cluster queued tasks; the rest is computed by the overflow kernel); the
    // consensus-word pipeline's deep queue shares the task array
    if (c->deep_sites_cap < pl->n_sites || c->deep_info_cap < (size_t)pl->n_sites * c->dp.n) {
        for (void *p : {(void *)c->deep.sites, (void *)c->deep.tasks, (void *)c->deep.info, (void *)c->deep.blk_cnt,
                        (void *)c->deep.raw, (void *)c->deep.pend})
            if (p) HIPCHK(c, hipFree(p));
        c->deep.blk_cnt = nullptr;
        c->deep.raw = nullptr;
        c->deep.pend = nullptr;
        c->deep.sites = nullptr;
        c->deep.tasks = nullptr;
        c->deep.info = nullptr;
        c->deep_sites_cap = c->deep_info_cap = 0;
        const size_t ntask = (size_t)pl->n_sites * c->dp.n;
        const uint32_t blk_cap = (uint32_t)(pbg::kSiteBlock * c->dp.n * 3 / 16 + 32);
        const size_t tcap = std::max<size_t>((size_t)nblk * blk_cap, std::min<size_t>(ntask / 32 + 65536, 0xFFFFFFFFu));
        HIPCHK(c, hipMalloc((void **)&c->deep.sites, (size_t)pl->n_sites * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc((void **)&c->deep.tasks, tcap * sizeof(pbg::DeepTask)));
        HIPCHK(c, hipMalloc((void **)&c->deep.info, ntask + 64));   // + slack: the scan's fold reads whole dwords
        HIPCHK(c, hipMalloc((void **)&c->deep.pend, (size_t)nblk * sizeof(uint64_t)));
        c->deep.task_cap = (uint32_t)std::min<size_t>(tcap, 0xFFFFFFFFu);
        c->deep.blk_cap = blk_cap;
        HIPCHK(c, hipMalloc((void **)&c->deep.blk_cnt, (size_t)nblk * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc((void **)&c->deep.raw, (size_t)nblk * blk_cap * 3 * sizeof(uint4)));
        c->deep_sites_cap = pl->n_sites;
        c->deep_info_cap = ntask;
        // allocated lengths, for the PBG_BOUNDS store checks
        c->deep.raw_n = c->deep.raw_chk = (uint64_t)nblk * blk_cap * 3;
        c->deep.info_n = c->deep.info_chk = ntask;
        c->deep.tasks_n = c->deep.tasks_chk = c->deep.task_cap;
        c->deep.blk_n = c->deep.blk_chk = nblk;
        c->deep.sites_n = c->deep.sites_chk = pl->n_sites;
    }
    if (!c->deep.count) HIPCHK(c, hipMalloc((void **)&c->deep.count, 4 * sizeof(uint32_t)));
    hipEvent_t e0 = nullptr, e1 = nullptr, c0 = nullptr, c1 = nullptr;
    if (c->timing) {
        if (c->ev_used == c->ev.size()) {
            hipEvent_t a, b, x, y;
            HIPCHK(c, hipEventCreate(&a));
            HIPCHK(c, hipEventCreate(&b));
            HIPCHK(c, hipEventCreate(&x));
            HIPCHK(c, hipEventCreate(&y));
            c->ev.emplace_back(a, b);
            c->evc.emplace_back(x, y);
        }
        e0 = c->ev[c->ev_used].first;
        e1 = c->ev[c->ev_used].second;
        c0 = c->evc[c->ev_used].first;
        c1 = c->evc[c->ev_used].second;
        ++c->ev_used;
        HIPCHK(c, hipEventRecord(c0, (hipStream_t)stream));
    }
    uint32_t shrink = 0;
    pbg::DeepBufs D = c->deep;
    D.rows_div = D.words_div = 1;
#ifdef PBG_BOUNDS
    // positive controls of the bounds build: PBG_BOUNDS_SELFTEST names the class whose checked
    // range is cut (keys: the batch's last chunk; queue / info / block: half the array; deep: all
    // of it; rows / words: half the batch; pool: pbg_window_stats), so correct kernels trip that
    // class's check
    if (const char *st = std::getenv("PBG_BOUNDS_SELFTEST")) {
        const std::string m = st;
        if (m == "1" || m == "keys") shrink = 8u;
        else if (m == "queue") D.raw_chk = D.raw_n / 2;
        else if (m == "info") D.info_chk = D.info_n / 2;
        else if (m == "deep") D.tasks_chk = 0;
        else if (m == "block") D.blk_chk = D.blk_n / 2;
        else if (m == "rows") D.rows_div = 2;
        else if (m == "words") D.words_div = 2;
    }
#endif
    if (cb && c->scan_compact) return fail(c, PBG_E_ARG, "compact pieces carry no keys for reference-only tasks: no consensus words");
    const pbg::Batch B{pl->n_sites, pl->ref, pl->k, pl->rmsq, pl->block_off, pl->keys, c->d_err, c->scan_masked, c->scan_compact,
                       shrink};
    HIPCHK(c, pbg::launch_call_sites(c->row_bytes, c->dp, c->dt, B, cap, rows, cb, c->d_err, D,
                                     (hipStream_t)stream, e0, e1, c->n_cu));
    if (c1) HIPCHK(c, hipEventRecord(c1, (hipStream_t)stream));
    return PBG_OK;
}

const char *pbg_build_info(void) {
    const int kind = std::max({(int)PBG_BUILD_KIND, pbg::kBuildKind_call, pbg::kBuildKind_stats, pbg::kBuildKind_decay,
                               pbg::kBuildKind_jsfs, pbg::kBuildKind_dstat, pbg::kBuildKind_hfs, pbg::kBuildKind_rmin,
                               pbg::kBuildKind_nsl, pbg::kBuildKind_xpnsl, pbg::kBuildKind_snn});
    return kind == 2 ? "experiment" : kind == 1 ? "bounds" : "product";
}

int pbg_check(pbg_ctx *c, void *stream) {
    if (!c) return fail(c, PBG_E_ARG, "null argument");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
    int herr = 0;
    HIPCHK(c, hipMemcpy(&herr, c->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (!herr) return PBG_OK;
    HIPCHK(c, hipMemset(c->d_err, 0, sizeof(int)));
    if (herr & 4) return fail(c, PBG_E_RANGE, "statistics workspace exhausted (windows with very many segregating sites)");
    if (herr & 8) return fail(c, PBG_E_BATCH, "a kernel loaded keys outside [block_off[0], block_off[last]) (PBG_BOUNDS build)");
    if (herr & pbg::kErrQueue) return fail(c, PBG_E_BATCH, "a queue record was stored outside its block's region of the queue (PBG_BOUNDS build)");
    if (herr & pbg::kErrDeep) return fail(c, PBG_E_BATCH, "a deep-task entry was stored outside the task list (PBG_BOUNDS build)");
    if (herr & pbg::kErrInfo) return fail(c, PBG_E_BATCH, "an info byte was stored outside the info array (PBG_BOUNDS build)");
    if (herr & pbg::kErrRow) return fail(c, PBG_E_BATCH, "a row was stored outside the batch's rows (PBG_BOUNDS build)");
    if (herr & pbg::kErrBlock) return fail(c, PBG_E_BATCH, "a block's pending mask / queue count / overflow entry was stored out of range (PBG_BOUNDS build)");
    if (herr & pbg::kErrWords) return fail(c, PBG_E_BATCH, "a consensus word was stored outside the batch's words (PBG_BOUNDS build)");
    if (herr & pbg::kErrCompact) return fail(c, PBG_E_BATCH, "a compact piece flagged a task that is not reference-only (1..32 keys on an upper-case A/C/G/T reference base)");
    if (herr & pbg::kErrPool) return fail(c, PBG_E_BATCH, "a statistics workspace store fell outside its pool slice (PBG_BOUNDS build)");
    if (herr & 2) return fail(c, PBG_E_BATCH, "synthetic batch needs more keys than keys_cap");
    return fail(c, PBG_E_BATCH, "pileup block_off disagrees with k[]");
}

int pbg_set_kernel_timing(pbg_ctx *c, int on) {
    if (!c) return fail(c, PBG_E_ARG, "null argument");
    c->timing = on != 0;
    c->ev_used = 0;
    return PBG_OK;
}

int pbg_kernel_time(pbg_ctx *c, double *ms_total, uint32_t *launches) {
    return event_time(c, &pbg_ctx::ev, ms_total, launches);
}

int pbg_call_time(pbg_ctx *c, double *ms_total, uint32_t *launches) {
    return event_time(c, &pbg_ctx::evc, ms_total, launches);
}

int pbg_window_stats(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                     const pbg_stat_opts *o, const pbg_window_out *out, void *stream) {
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    if (n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    {
        const uint32_t ld = o->stats & (PBG_S_ZNS | PBG_S_OMEGA | PBG_S_WALL);
        if (ld & (ld - 1)) return fail(c, PBG_E_ARG, "at most one of ZnS / omega / Wall per call (shared outputs)");
    }
    HIPCHK(c, hipSetDevice(c->device));
    pbg::StatsArgs A{};
    A.pool_div = 1;
#ifdef PBG_BOUNDS
    if (const char *st = std::getenv("PBG_BOUNDS_SELFTEST"))
        if (std::string(st) == "pool") A.pool_div = 2;   // positive control of the pool store checks
#endif
    A.stats = o->stats;
    A.min_freq = o->min_freq;
    A.outidx = o->outidx;
    A.jc = o->jc;
    A.wins = wins;
    A.out = *out;
    // statistics workspace: a pool the windows take slices of on the device (windows with more
    // than kSegCap segregating rows, omega / Wall lists, ZnS lists).  Sized from the window list
    // (worst case, at most kPoolMax words); the plan is cached per device window list, so
    // steady-state calls do not synchronise.
    const bool ld_ws = (o->stats & (PBG_S_OMEGA | PBG_S_WALL)) != 0;
    const int n = c->dp.n, np = c->dp.npops;
    const uint64_t mw = c->row_bytes == 16 ? 2 : 1;
    bool known = false;
    uint64_t zstride = 0;
    int segcap = pbg::kSegCap;
    for (const auto &pl : c->plans)
        if (pl.wins == (const void *)wins && pl.n_win == n_win && pl.n_rows == n_rows && pl.stats == o->stats) {
            known = true;
            zstride = pl.zstride;
            segcap = pl.segcap;
        }
    if (!known) {
        std::vector<pbg_window> hw;
        if (int rc = fetch_windows(c, wins, n_win, (hipStream_t)stream, hw)) return rc;
        uint64_t worst = 0, maxlen = 0;
        for (uint32_t i = 0; i < n_win; ++i) {
            if (hw[i].beg < 0 || hw[i].end < hw[i].beg || (uint32_t)hw[i].end > n_rows)
                return fail(c, PBG_E_RANGE, "window outside the row range");
            maxlen = std::max<uint64_t>(maxlen, (uint64_t)(hw[i].end - hw[i].beg));
        }
        // segregating rows each window keeps in LDS: short windows need few, and a smaller slice
        // leaves room for more waves per CU (1 kb windows at 96 samples: 64 rows, 1 KB of masks);
        // windows with more spill to the pool
        segcap = maxlen <= 2048 ? 64 : maxlen <= 8192 ? 128 : pbg::kSegCap;
        for (uint32_t i = 0; i < n_win; ++i) {
            const uint64_t len = (uint64_t)(hw[i].end - hw[i].beg);
            // words: masks are mw words each (two for 16-byte rows)
            if (ld_ws || len > (uint64_t)segcap) worst += mw * len + (uint64_t)n * (len / 64 + 1) + (ld_ws ? mw * np * len : 0);
            if (o->stats & PBG_S_ZNS) worst += mw * np * len;
        }
        if (int rc = size_pool(c, worst)) return rc;
        // win_off | zoff | pool_used
        if (int rc = pbg::grow(c, c->wsoff, (size_t)n_win * 16 + (size_t)n_win * np * 8 + 8)) return rc;
        // seg_count [n_win] | var_count [n_win*np] | ld_ns [n_win*np]
        if (int rc = pbg::grow(c, c->segcnt, (size_t)n_win * (1 + 2 * (size_t)np) * 4)) return rc;
        // ZnS lists at fixed places (no pool allocation in the kernel) when windows are of
        // (nearly) one length: n_win * npops * maxlen words, at most twice the exact need
        if (o->stats & PBG_S_ZNS) {
            uint64_t need = 0;
            for (uint32_t i = 0; i < n_win; ++i) need += mw * np * (uint64_t)(hw[i].end - hw[i].beg);
            const uint64_t zs = mw * np * std::max<uint64_t>(maxlen, 1);
            if ((uint64_t)n_win * zs <= std::max<uint64_t>(2 * need, 1 << 20) && (uint64_t)n_win * zs <= kPoolMax) {
                zstride = zs;
                if (int rc = pbg::grow(c, c->zns, (size_t)n_win * zs * 8)) return rc;
            }
        }
        if (c->plans.size() >= 16) c->plans.erase(c->plans.begin());
        c->plans.push_back({wins, n_win, n_rows, o->stats, zstride, segcap});
    }
    A.pool = (uint64_t *)c->ws.d;
    A.pool_cap = c->ws.cap / 8;
    A.win_off = (uint64_t *)c->wsoff.d;
    A.zoff = A.win_off + 2 * (size_t)n_win;
    A.pool_used = reinterpret_cast<unsigned long long *>(A.zoff + (size_t)n_win * np);
    A.err = c->d_err;
    HIPCHK(c, hipMemsetAsync(A.pool_used, 0, 8, (hipStream_t)stream));
    A.zlist = (uint64_t *)c->zns.d;
    A.zstride = zstride;
    A.seg_count = (int32_t *)c->segcnt.d;
    A.var_count = A.seg_count + n_win;
    A.ld_ns = A.var_count + (size_t)n_win * np;
    A.lds = pbg::stats_lds_layout(n, np, c->dp.sfs_stride, o->stats, 0, (int)mw, segcap);
    if (A.lds.bytes > 64 * 1024) return fail(c, PBG_E_ARG, "statistics need more LDS than a workgroup has");
    HIPCHK(c, pbg::launch_window_stats(c->row_bytes, c->dp, c->dt, rows, n_rows, n_win, A, (hipStream_t)stream, c->n_cu));
    return PBG_OK;
}

int pbg_window_ld_decay(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                        const pbg_decay_opts *o, const pbg_decay_out *out, void *stream) {
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    if (o->bin_bp < 1) return fail(c, PBG_E_ARG, "decay: bin_bp must be at least 1");
    if (o->n_bins < 1 || o->n_bins > PBG_DECAY_MAX_BINS) return fail(c, PBG_E_ARG, "decay: n_bins must be in [1, 256]");
    if (o->min_freq != 1 && o->min_freq != 2) return fail(c, PBG_E_ARG, "decay: min_freq must be 1 or 2");
    if (n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    const int np = c->dp.npops;
    if ((uint64_t)n_win * (uint64_t)np > 0x7FFFFFFFull) return fail(c, PBG_E_ARG, "decay: too many windows");
    HIPCHK(c, hipSetDevice(c->device));
    pbg::DecayArgs A{};
    A.pool_div = 1;
#ifdef PBG_BOUNDS
    if (const char *st = std::getenv("PBG_BOUNDS_SELFTEST"))
        if (std::string(st) == "pool") A.pool_div = 2;   // positive control of the pool store checks
#endif
    A.wins = wins;
    A.bin_bp = o->bin_bp;
    A.n_bins = o->n_bins;
    A.min_freq = o->min_freq;
    const size_t lds = pbg::decay_lds_bytes(c->row_bytes, c->dp, A);
    // The workspace is the pool pbg_window_stats uses (size_pool), sized from the window list (every
    // window longer than the LDS list capacity, all rows variable); validated lists are cached per
    // device pointer like the statistics plans.
    bool known = false;
    for (const auto &pl : c->decay_plans)
        if (pl.wins == (const void *)wins && pl.n_win == n_win && pl.n_rows == n_rows) known = true;
    if (!known) {
        std::vector<pbg_window> hw;
        if (int rc = fetch_windows(c, wins, n_win, (hipStream_t)stream, hw)) return rc;
        const uint64_t mw = c->row_bytes == 16 ? 2 : 1;
        uint64_t worst = 0;
        for (uint32_t i = 0; i < n_win; ++i) {
            if (hw[i].beg < 0 || (hw[i].end > hw[i].beg && (uint32_t)hw[i].end > n_rows))
                return fail(c, PBG_E_RANGE, "window outside the row range");
            const uint64_t len = hw[i].end > hw[i].beg ? (uint64_t)(hw[i].end - hw[i].beg) : 0;
            if (len > (uint64_t)pbg::kDecayCap) worst += (uint64_t)np * (A.compact ? len : mw * len + (len + 1) / 2);
        }
        if (int rc = size_pool(c, worst)) return rc;
        if (c->decay_plans.size() >= 16) c->decay_plans.erase(c->decay_plans.begin());
        c->decay_plans.push_back({wins, n_win, n_rows});
    }
    if (!c->d_decay_used) HIPCHK(c, hipMalloc((void **)&c->d_decay_used, 8));
    A.pool = (uint64_t *)c->ws.d;
    A.pool_cap = c->ws.cap / 8;
    A.pool_used = c->d_decay_used;
    A.err = c->d_err;
    A.pairs = out->pairs;
    A.r2_sum = out->r2_sum;
    A.n_var = out->n_var;
    HIPCHK(c, hipMemsetAsync(A.pool_used, 0, 8, (hipStream_t)stream));
    HIPCHK(c, pbg::launch_window_decay(c->row_bytes, c->dp, c->dt, rows, n_rows, n_win, A, lds, (hipStream_t)stream));
    return PBG_OK;
}

int pbg_jsfs_cells(const pbg_ctx *c) { return c ? jsfs_offsets(c->dp).back() : 0; }

int pbg_jsfs_pair_offset(const pbg_ctx *c, int i, int j) {
    if (!c) return PBG_E_ARG;
    const int np = c->dp.npops;
    if (i < 0 || j <= i || j >= np) return PBG_E_ARG;
    return jsfs_offsets(c->dp)[(size_t)(i * (2 * np - i - 1) / 2 + (j - i - 1))];
}

int pbg_window_jsfs(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                    const pbg_jsfs_opts *o, const pbg_jsfs_out *out, void *stream) {
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    int32_t flip_idx;
    if (int rc = check_outidx(c, "jsfs", o->outidx, &flip_idx)) return rc;
    const int np = c->dp.npops;
    if (np < 2 || n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    pbg_ctx::JsfsPlan &pl = c->jsfs;
    HIPCHK(c, hipSetDevice(c->device));
    if (!pl.built) {
        // the counts are popcounts within the masks, so the cell layout (from pop_n) needs them equal
        if (int rc = check_pop_sizes(c, "jsfs")) return rc;
        const std::vector<int32_t> off = jsfs_offsets(c->dp);
        std::vector<uint32_t> pairs;
        for (int i = 0; i < np; ++i)
            for (int j = i + 1; j < np; ++j) pairs.push_back(pbg::jsfs_pair_word((uint32_t)off[pairs.size()], i, j));
        // groups of consecutive pairs whose cells fit the LDS histogram (one pair always does)
        std::vector<int32_t> groups{0};
        int32_t lds_cells = 0;
        for (size_t p = 0, g0 = 0; p < pairs.size(); ++p) {
            if (off[p + 1] - off[g0] > pbg::kJsfsLdsCells) {
                groups.push_back((int32_t)p);
                g0 = p;
            }
            lds_cells = std::max(lds_cells, off[p + 1] - off[g0]);
        }
        groups.push_back((int32_t)pairs.size());
        HIPCHK(c, hipMalloc((void **)&pl.d_pairs, pairs.size() * 4));
        HIPCHK(c, hipMalloc((void **)&pl.d_groups, groups.size() * 4));
        HIPCHK(c, hipMemcpy(pl.d_pairs, pairs.data(), pairs.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(pl.d_groups, groups.data(), groups.size() * 4, hipMemcpyHostToDevice));
        pl.n_pairs = (int32_t)pairs.size();
        pl.n_groups = (int32_t)groups.size() - 1;
        pl.n_cells = off.back();
        pl.lds_cells = lds_cells;
        pl.built = true;
    }
    if ((uint64_t)n_win * (uint64_t)pl.n_cells > 0x7FFFFFFFull || (uint64_t)n_win * (uint64_t)pl.n_pairs > 0x7FFFFFFFull)
        return fail(c, PBG_E_ARG, "jsfs: too many windows");
    pbg::JsfsArgs A{};
    A.wins = wins;
    A.pairs = pl.d_pairs;
    A.groups = pl.d_groups;
    A.n_pairs = pl.n_pairs;
    A.n_groups = pl.n_groups;
    A.n_cells = pl.n_cells;
    A.lds_cells = pl.lds_cells;
    A.outidx = flip_idx;
    A.err = c->d_err;
    A.cells = out->cells;
    A.diffs = out->diffs;
    A.fst = out->fst;
    HIPCHK(c, pbg::launch_window_jsfs(c->row_bytes, c->dp, rows, n_rows, n_win, A, (hipStream_t)stream));
    return PBG_OK;
}

int pbg_window_dstat(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                     const pbg_dstat_opts *o, const pbg_dstat_out *out, void *stream) {
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    if (o->n_triples < 0 || o->n_triples > PBG_DSTAT_MAX_TRIPLES)
        return fail(c, PBG_E_ARG, "dstat: n_triples must be in [0, " + std::to_string(PBG_DSTAT_MAX_TRIPLES) + "]");
    if (o->n_triples > 0 && !o->triples) return fail(c, PBG_E_ARG, "dstat: null triple list");
    int32_t flip_idx;
    if (int rc = check_outidx(c, "dstat", o->outidx, &flip_idx)) return rc;
    const int np = c->dp.npops;
    std::vector<uint32_t> words((size_t)o->n_triples);
    for (int t = 0; t < o->n_triples; ++t) {
        const pbg_triple &tr = o->triples[t];
        if (tr.p1 < 0 || tr.p1 >= np || tr.p2 < 0 || tr.p2 >= np || tr.p3 < 0 || tr.p3 >= np)
            return fail(c, PBG_E_ARG, "dstat: triple " + std::to_string(t) + " names a population outside 0.." + std::to_string(np - 1));
        if (tr.p1 == tr.p2 || tr.p1 == tr.p3 || tr.p2 == tr.p3)
            return fail(c, PBG_E_ARG, "dstat: the populations of triple " + std::to_string(t) + " are not distinct");
        words[(size_t)t] = pbg::dstat_triple_word(tr.p1, tr.p2, tr.p3);
    }
    if (o->n_triples == 0 || n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    // the counts are popcounts within the masks and are parked as bytes: n - count needs pop_n to be them
    if (int rc = check_pop_sizes(c, "dstat")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // the list's device copy, by content (pbg_ctx.h): written once, never overwritten
    const uint32_t *d_words = nullptr;
    for (size_t k = c->dstat_lists.size(); k-- > 0 && !d_words;)
        if (c->dstat_lists[k].words == words) {
            d_words = c->dstat_lists[k].d;
            std::rotate(c->dstat_lists.begin() + k, c->dstat_lists.begin() + k + 1, c->dstat_lists.end());
        }
    if (!d_words) {
        if (c->dstat_lists.size() >= 16) {
            HIPCHK(c, hipFree(c->dstat_lists.front().d));   // waits for every launch that may read it
            c->dstat_lists.erase(c->dstat_lists.begin());
        }
        uint32_t *d = nullptr;
        HIPCHK(c, hipMalloc((void **)&d, words.size() * 4));
        const hipError_t e = hipMemcpy(d, words.data(), words.size() * 4, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            HIPCHK(c, e);
        }
        c->dstat_lists.push_back({std::move(words), d});
        d_words = d;
    }
    pbg::DstatArgs A{};
    A.wins = wins;
    A.triples = d_words;
    A.n_triples = o->n_triples;
    A.outidx = flip_idx;
    A.err = c->d_err;
    A.sums = out->sums;
    A.d = out->d;
    A.fd = out->fd;
    A.fdm = out->fdm;
    HIPCHK(c, pbg::launch_window_dstat(c->row_bytes, c->dp, rows, n_rows, n_win, A, (hipStream_t)stream));
    return PBG_OK;
}

int pbg_window_hfs(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                   const pbg_hfs_out *out, void *stream) {
    if (!c || !rows || !wins || !out) return fail(c, PBG_E_ARG, "null argument");
    // a class label is a rank inside pop_mask and the doubles divide by pop_n: they must agree.  (A sample
    // in two populations cannot get here: pbg_create refuses overlapping masks.)
    if (int rc = check_pop_sizes(c, "hfs")) return rc;
    if (n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    pbg::HfsArgs A{};
    A.wins = wins;
    A.err = c->d_err;
    A.k = out->k;
    A.counts = out->counts;
    A.cls = out->cls;
    A.sums = out->sums;
    A.h = out->h;
    HIPCHK(c, pbg::launch_window_hfs(c->row_bytes, c->dp, rows, n_rows, n_win, A, (hipStream_t)stream));
    return PBG_OK;
}

int pbg_window_rmin(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                    const pbg_rmin_opts *o, const pbg_rmin_out *out, void *stream) {
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    if (o->min_freq != 1 && o->min_freq != 2) return fail(c, PBG_E_ARG, "rmin: min_freq must be 1 or 2");
    if (o->max_cuts < 0) return fail(c, PBG_E_ARG, "rmin: max_cuts must not be negative");
    if (out->cuts && o->max_cuts == 0) return fail(c, PBG_E_ARG, "rmin: cuts needs max_cuts of at least 1");
    if (n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    pbg::RminArgs A{};
    A.wins = wins;
    A.err = c->d_err;
    A.min_freq = o->min_freq;
    A.max_cuts = o->max_cuts;
    A.rmin = out->rmin;
    A.n_var = out->n_var;
    A.cuts = out->cuts;
    HIPCHK(c, pbg::launch_window_rmin(c->row_bytes, c->dp, rows, n_rows, n_win, A, (hipStream_t)stream));
    return PBG_OK;
}

int pbg_window_nsl(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                   const pbg_nsl_opts *o, const pbg_nsl_out *out, void *stream) {
    return window_tract(c, "nsl", 0, rows, n_rows, wins, n_win, o, out, stream, pbg::launch_window_nsl);
}

// one population has no pair: nothing is written
int pbg_window_xpnsl(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                     const pbg_xpnsl_opts *o, const pbg_xpnsl_out *out, void *stream) {
    return window_tract(c, "xpnsl", 2, rows, n_rows, wins, n_win, o, out, stream, pbg::launch_window_xpnsl);
}

int pbg_snn_chunks(uint32_t n_win, int32_t n_groups, int32_t n_perms) { return pbg::snn_chunks(n_win, n_groups, n_perms); }

int pbg_window_snn(pbg_ctx *c, const void *rows, uint32_t n_rows, const pbg_window *wins, uint32_t n_win,
                   const pbg_snn_opts *o, const pbg_snn_out *out, void *stream) {
    if (!c || !rows || !wins || !o || !out) return fail(c, PBG_E_ARG, "null argument");
    if (o->n_groups < 0 || o->n_groups > PBG_SNN_MAX_GROUPS)
        return fail(c, PBG_E_ARG, "snn: n_groups must be in [0, " + std::to_string(PBG_SNN_MAX_GROUPS) + "]");
    if (o->n_perms < 0 || o->n_perms > PBG_SNN_MAX_PERMS)
        return fail(c, PBG_E_ARG, "snn: n_perms must be in [0, " + std::to_string(PBG_SNN_MAX_PERMS) + "]");
    if (o->n_groups > 0 && !o->groups) return fail(c, PBG_E_ARG, "snn: null group list");
    const int np = c->dp.npops, ng = o->n_groups;
    std::vector<uint64_t> groups((size_t)ng);
    for (int g = 0; g < ng; ++g) {
        const uint64_t m = o->groups[g];
        if (np < 64 && (m >> np) != 0)
            return fail(c, PBG_E_ARG, "snn: group " + std::to_string(g) + " names a population outside 0.." + std::to_string(np - 1));
        if (__builtin_popcountll(m) < 2)
            return fail(c, PBG_E_ARG, "snn: group " + std::to_string(g) + " has fewer than two populations");
        groups[(size_t)g] = m;
    }
    if (ng > 0)   // the members come from pop_mask, the labels' count from pop_n
        if (int rc = check_pop_sizes(c, "snn")) return rc;
    if (n_win == 0) return PBG_OK;
    if ((uintptr_t)rows & 15) return fail(c, PBG_E_ARG, "rows must be 16-byte aligned");
    const int n = c->dp.n;
    const uint64_t npairs = (uint64_t)n * (uint64_t)(n - 1) / 2;
    const bool stat = ng > 0 && (out->snn || out->near || out->ge);
    if (!out->diff && !stat) return PBG_OK;   // nothing is wanted
    const int chunks = out->ge ? pbg::snn_chunks(n_win, ng, o->n_perms) : 1;
    if ((uint64_t)n_win * npairs > 0x7FFFFFFFull || (uint64_t)n_win * (uint64_t)std::max(ng, 1) * (uint64_t)chunks > 0x7FFFFFFFull)
        return fail(c, PBG_E_ARG, "snn: too many windows");
    HIPCHK(c, hipSetDevice(c->device));
    pbg::SnnArgs A{};
    A.wins = wins;
    A.err = c->d_err;
    A.n_pairs = (int32_t)npairs;
    A.diff = out->diff;
    if (!A.diff) {
        if (int rc = pbg::grow(c, c->snn_diff, std::max<size_t>((size_t)n_win * (size_t)npairs * 4, 16))) return rc;
        A.diff = (int32_t *)c->snn_diff.d;
    }
    if (stat) {
        // the list's device copy, by content (pbg_ctx.h): written once, never overwritten
        const uint64_t *d_groups = nullptr;
        for (size_t k = c->snn_lists.size(); k-- > 0 && !d_groups;)
            if (c->snn_lists[k].groups == groups) {
                d_groups = c->snn_lists[k].d;
                std::rotate(c->snn_lists.begin() + k, c->snn_lists.begin() + k + 1, c->snn_lists.end());
            }
        if (!d_groups) {
            if (c->snn_lists.size() >= 16) {
                HIPCHK(c, hipFree(c->snn_lists.front().d));   // waits for every launch that may read it
                c->snn_lists.erase(c->snn_lists.begin());
            }
            uint64_t *d = nullptr;
            HIPCHK(c, hipMalloc((void **)&d, groups.size() * 8));
            const hipError_t e = hipMemcpy(d, groups.data(), groups.size() * 8, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                (void)hipFree(d);
                HIPCHK(c, e);
            }
            c->snn_lists.push_back({std::move(groups), d});
            d_groups = d;
        }
        A.groups = d_groups;
        A.n_groups = ng;
        A.n_perms = o->n_perms;
        A.chunks = chunks;
        A.per_chunk = (o->n_perms + chunks - 1) / chunks;
        A.seed = o->seed;
        A.key0 = o->key0;
        A.snn = out->snn;
        A.near = out->near;
        A.ge = out->ge;
        if (A.ge) HIPCHK(c, hipMemsetAsync(A.ge, 0, (size_t)n_win * (size_t)ng * 4, (hipStream_t)stream));
    }
    HIPCHK(c, pbg::launch_window_pairdiff(c->row_bytes, c->dp, rows, n_rows, n_win, A, (hipStream_t)stream));
    if (stat) HIPCHK(c, pbg::launch_window_snn(c->dp, n_win, A, (hipStream_t)stream));
    return PBG_OK;
}

uint64_t pbg_synth_max_keys(const pbg_ctx *c, const pbg_synth_spec *sp) {
    if (!c || !sp) return 0;
    const int dmax = std::min(2 * sp->mean_depth, c->dp.max_depth);
    return (uint64_t)sp->n_sites * (uint64_t)c->dp.n * (uint64_t)std::max(dmax, 0);
}

int pbg_synth_pileup(pbg_ctx *c, const pbg_synth_spec *sp, uint8_t *ref, void *k, uint32_t *rmsq, uint64_t *block_off,
                     uint16_t *keys, uint64_t keys_cap, uint64_t *n_keys, void *stream) {
    if (!c || !sp || !ref || !k || !rmsq || !block_off || (!keys && keys_cap)) return fail(c, PBG_E_ARG, "null argument");
    if (sp->mean_depth < 1 || sp->mean_depth > 32) return fail(c, PBG_E_ARG, "mean_depth must be in [1, 32]");
    if (((uintptr_t)keys | (uintptr_t)k | (uintptr_t)rmsq | (uintptr_t)ref) & 15)
        return fail(c, PBG_E_ARG, "keys / k / rmsq / ref must be 16-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t s = (hipStream_t)stream;
    const uint16_t *tmpl = nullptr;
    for (auto &t : c->tmpl)
        if (t.first == sp->seed) tmpl = t.second;
    if (!tmpl) {   // first use of this seed: build its table and wait for it (every stream may read it)
        constexpr size_t kTmplCache = 8;   // tables kept per context (2 MB each)
        if (c->tmpl.size() >= kTmplCache) {   // evict the oldest once no launch can still read it
            HIPCHK(c, hipDeviceSynchronize());
            HIPCHK(c, hipFree(c->tmpl.front().second));
            c->tmpl.erase(c->tmpl.begin());
        }
        uint16_t *t = nullptr;
        HIPCHK(c, hipMalloc((void **)&t, pbg::kTmplSize * sizeof(uint16_t)));
        hipError_t e = pbg::launch_synth_tmpl(sp->seed, t, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {   // never cache a table that was not built
            (void)hipFree(t);
            return fail(c, PBG_E_HIP, std::string("synthetic template table: ") + hipGetErrorString(e));
        }
        c->tmpl.emplace_back(sp->seed, t);   // cached only once built
        tmpl = t;
    }
    if (int rc = pbg::grow(c, c->synth, pbg::synth_scratch_words(sp->n_sites) * 8)) return rc;
    HIPCHK(c, pbg::launch_synth(c->dp, sp->seed, sp->contig, sp->mean_depth, sp->pos0, sp->n_sites, ref, k, rmsq,
                                block_off, keys, keys_cap, (uint64_t *)c->synth.d, tmpl, c->d_err, s));
    if (n_keys) {
        const uint32_t nblk = (sp->n_sites + pbg::kSiteBlock - 1) / pbg::kSiteBlock;
        HIPCHK(c, hipMemcpyAsync(n_keys, block_off + nblk, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        int rc = pbg_check(c, stream);
        if (rc) return rc;
    }
    return PBG_OK;
}

long pbg_format(const pbg_ctx *c, const pbg_cmd *cmd, const pbg_window_out *ho, uint32_t n_win, const int32_t *wbeg,
                const int32_t *wend, char *out, size_t cap, size_t *needed) {
    if (!c || !cmd || !ho || !wbeg || !wend || (!out && cap)) return fail(const_cast<pbg_ctx *>(c), PBG_E_ARG, "null argument");
    const int n = c->dp.n, np = c->dp.npops, npairs = std::max(1, np * (np - 1));
    std::string text;
    pbg::WindowHost wh;
    auto take = [](auto *src, size_t off, size_t cnt) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
        return src ? std::vector<T>(src + off, src + off + cnt) : std::vector<T>(cnt, T());
    };
    for (uint32_t i = 0; i < n_win; ++i) {
        wh.beg = wbeg[i];
        wh.end = wend[i];
        wh.num_sites = ho->num_sites ? ho->num_sites[i] : 0;
        wh.segsites = ho->segsites ? ho->segsites[i] : 0;
        wh.pi = take(ho->pi, (size_t)i * np, np);
        wh.dxy = take(ho->dxy, (size_t)i * npairs, npairs);
        wh.td = take(ho->td, (size_t)i * np, np);
        wh.fwh = take(ho->fwh, (size_t)i * np, np);
        wh.ld_snps = take(ho->ld_snps, (size_t)i * np, np);
        wh.ld_val = take(ho->ld_val, (size_t)i * np, np);
        wh.ld_q = take(ho->ld_q, (size_t)i * np, np);
        wh.div_ind = take(ho->div_ind, (size_t)i * n, n);
        wh.div_fixed = take(ho->div_fixed, (size_t)i * np, np);
        wh.div_seg = take(ho->div_seg, (size_t)i * np, np);
        wh.div_pop = take(ho->div_pop, (size_t)i * np, np);
        wh.nhaps = take(ho->nhaps, (size_t)i * np, np);
        wh.hap_val = take(ho->hap_val, (size_t)i * np, np);
        wh.hap_dxy = take(ho->hap_dxy, (size_t)i * npairs, npairs);
        wh.hap_min = take(ho->hap_min, (size_t)i * npairs, npairs);
        wh.tree_diff = take(ho->tree_diff, (size_t)i * (n + 1) * (n + 1), (size_t)(n + 1) * (n + 1));
        if (cmd->cmd == PBG_CMD_SFS && (cmd->output & 1) && ho->seg_pop && ho->theta_w && ho->sfs_bins) {
            wh.seg_pop = take(ho->seg_pop, (size_t)i * np, np);
            wh.theta_w = take(ho->theta_w, (size_t)i * np, np);
            wh.sfs_bins.assign(np, {});
            for (int p = 0; p < np; ++p)
                wh.sfs_bins[p] = take(ho->sfs_bins, ((size_t)i * np + p) * c->dp.sfs_stride, (size_t)c->dp.pop_n[p] + 1);
        }
        pbg::format_window(text, *cmd, n, np, c->dp.flag, wh);
    }
    if (needed) *needed = text.size() + 1;
    if (text.size() + 1 > cap) return fail(const_cast<pbg_ctx *>(c), PBG_E_RANGE, "output buffer too small");
    std::memcpy(out, text.c_str(), text.size() + 1);
    return (long)text.size();
}

}  // extern "C"
