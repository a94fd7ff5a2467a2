// format.cpp -- TSV writer, byte-identical to the reference's print_<stat> functions.
//
// The reference streams to std::cout with `std::fixed << std::setprecision(5)` (sticky),
// which libstdc++ renders through printf's "%.5f"; "NA" cells are `"\t" << std::setw(7) <<
// "NA"`, i.e. five spaces then NA.  Integers print in decimal.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "pbg_host.h"

namespace pbg {

namespace {

struct W {
    std::string &s;
    void t(const char *x) { s += x; }
    void t(const std::string &x) { s += x; }
    void i(long long v) { s += std::to_string(v); }
    void f(double v) {
        char b[400];
        std::snprintf(b, sizeof b, "%.5f", v);
        s += b;
    }
    void na() { s += "     NA"; }
};

std::string pn(const pbg_cmd &c, int i) { return c.pop_names[i]; }

// ---- tree (pop_tree.cpp): distances, neighbour joining and the Newick printer.
// The tree is O(ntaxa^3) scalar work on an (n+1)x(n+1) matrix per window, so it runs on the
// host on the GPU's diff_matrix.  Nodes live in one array; a ring of three nodes is one
// internal node as in tree_init (pop_tree.cpp:517-539), -1 is the null pointer.
struct NjNode {
    int next = -1, back = -1, index = 0;
    bool tip = false;
    double v = 0.0;
};

struct Nj {
    int ntaxa;
    std::vector<NjNode> nd;
    std::vector<int> nodep;   // curtree.nodep

    explicit Nj(int nt) : ntaxa(nt) {
        const int nnodes = 2 * nt - 1;
        nodep.resize(nnodes);
        for (int i = 0; i < nnodes; ++i) {
            const int h = (int)nd.size();
            if (i < nt) {
                nd.emplace_back();
            } else {   // ring head -> a -> b -> head
                nd.resize(nd.size() + 3);
                nd[h].next = h + 1;
                nd[h + 1].next = h + 2;
                nd[h + 2].next = h;
            }
            nodep[i] = h;
        }
        nd[nodep[nnodes - 1]].next = nodep[nnodes - 1];   // make_nj: last ring cut to one node
        for (int i = 1; i <= nnodes; ++i) {                // setup_tree pop_tree.cpp:541-566
            NjNode &q = nd[nodep[i - 1]];
            q.back = -1;
            q.tip = i <= nt;
            q.index = i;
            q.v = 0.0;
            if (i > nt)
                for (int r = q.next; r != nodep[i - 1]; r = nd[r].next) {
                    nd[r].back = -1;
                    nd[r].tip = false;
                    nd[r].index = i;
                }
        }
    }
    void hookup(int p, int q) {
        nd[p].back = q;
        nd[q].back = p;
    }
    void set_len(int c, double v) {
        nd[c].v = v;
        nd[nd[c].back].v = v;
    }

    // join_tree pop_tree.cpp:254-429, statement for statement (including `total` carried over
    // from a skipped pair and across cycles, and the column sums over cleared rows)
    void join(std::vector<double> x) {
        const int nt = ntaxa;
        auto X = [&](int i, int j) -> double & { return x[(size_t)i * nt + j]; };
        std::vector<int> cluster(nt), eo(nt);
        std::vector<double> av(nt, 0.0), R(nt);
        for (int i = 0; i < nt; ++i) {
            cluster[i] = nodep[i];
            eo[i] = i + 1;
        }
        for (int i = 0; i < nt - 1; i++)
            for (int j = i + 1; j < nt; j++) {
                const double da = (X(i, j) + X(j, i)) / 2.0;
                X(i, j) = da;
                X(j, i) = da;
            }
        double fotu2 = nt - 2.0, total = 0, tmin, dio, djo, bi, bj, bk, dmin;
        int nextnode = nt + 1, mini = 0, minj = 0;
        for (int nc = 1; nc <= nt - 3; nc++) {
            for (int j = 2; j <= nt; j++)
                for (int i = 0; i <= j - 2; i++) X(j - 1, i) = X(i, j - 1);
            tmin = DBL_MAX;
            for (int i = 0; i < nt; i++) R[i] = 0.0;
            for (int ja = 2; ja <= nt; ja++) {
                const int jj = eo[ja - 1];
                if (cluster[jj - 1] < 0) continue;
                for (int ia = 0; ia <= ja - 2; ia++) {
                    const int ii = eo[ia];
                    if (cluster[ii - 1] >= 0) {
                        R[ii - 1] += X(ii - 1, jj - 1);
                        R[jj - 1] += X(ii - 1, jj - 1);
                    }
                }
            }
            for (int ja = 2; ja <= nt; ja++) {
                const int jj = eo[ja - 1];
                if (cluster[jj - 1] < 0) continue;
                for (int ia = 0; ia <= ja - 2; ia++) {
                    const int ii = eo[ia];
                    if (cluster[ii - 1] >= 0) total = fotu2 * X(ii - 1, jj - 1) - R[ii - 1] - R[jj - 1];
                    if (total < tmin) {
                        tmin = total;
                        mini = ii;
                        minj = jj;
                    }
                }
            }
            dio = 0.0;
            djo = 0.0;
            for (int i = 0; i < nt; i++) {
                dio += X(i, mini - 1);
                djo += X(i, minj - 1);
            }
            dmin = X(mini - 1, minj - 1);
            dio = (dio - dmin) / fotu2;
            djo = (djo - dmin) / fotu2;
            bi = (dmin + dio - djo) * 0.5;
            bj = dmin - bi;
            bi -= av[mini - 1];
            bj -= av[minj - 1];
            const int h = nodep[nextnode - 1];
            hookup(nd[h].next, cluster[mini - 1]);
            hookup(nd[nd[h].next].next, cluster[minj - 1]);
            set_len(cluster[mini - 1], bi);
            set_len(cluster[minj - 1], bj);
            cluster[mini - 1] = h;
            cluster[minj - 1] = -1;
            nextnode++;
            av[mini - 1] = dmin * 0.5;
            fotu2 -= 1.0;
            for (int j = 0; j < nt; j++)
                if (cluster[j] >= 0) {
                    const double da = (X(mini - 1, j) + X(minj - 1, j)) * 0.5;
                    if (mini - j - 1 < 0) X(mini - 1, j) = da;
                    if (mini - j - 1 > 0) X(j, mini - 1) = da;
                }
            for (int j = 0; j < nt; j++) {
                X(minj - 1, j) = 0.0;
                X(j, minj - 1) = 0.0;
            }
        }
        int el[3] = {0, 0, 0}, nude = 1;
        for (int i = 1; i <= nt && nude <= 3; i++)
            if (cluster[i - 1] >= 0) el[nude++ - 1] = i;
        bi = (X(el[0] - 1, el[1] - 1) + X(el[0] - 1, el[2] - 1) - X(el[1] - 1, el[2] - 1)) * 0.5;
        bj = X(el[0] - 1, el[1] - 1) - bi;
        bk = X(el[0] - 1, el[2] - 1) - bi;
        bi -= av[el[0] - 1];
        bj -= av[el[1] - 1];
        bk -= av[el[2] - 1];
        const int h = nodep[nextnode - 1];
        hookup(h, cluster[el[0] - 1]);
        hookup(nd[h].next, cluster[el[1] - 1]);
        hookup(nd[nd[h].next].next, cluster[el[2] - 1]);
        set_len(cluster[el[0] - 1], bi);
        set_len(cluster[el[1] - 1], bj);
        set_len(cluster[el[2] - 1], bk);
    }

    // print_tree pop_tree.cpp:439-470
    void print(W &o, int p, int start, const char *refid, const char *const *names) const {
        const NjNode &q = nd[p];
        if (q.tip) {
            o.t(q.index == 1 ? refid : names[q.index - 2]);
        } else {
            o.t("(");
            print(o, nd[q.next].back, start, refid, names);
            o.t(",");
            print(o, nd[nd[q.next].next].back, start, refid, names);
            if (p == start) {
                o.t(",");
                print(o, q.back, start, refid, names);
            }
            o.t(")");
        }
        if (p == start) {
            o.t(";");
        } else if (q.v < 0) {
            o.t(":0.00000");
        } else {
            o.t(":");
            o.f(q.v);
        }
    }
};

// make_nj pop_tree.cpp:208-252 after calc_dist_matrix 496-515 (the caller prints the row head)
void format_nj(W &o, const pbg_cmd &c, int n, const WindowHost &w) {
    if (w.num_sites < c.min_sites || w.segsites < 1) {
        o.t("\tNA");
        return;
    }
    const int nt = n + 1;
    std::vector<double> dist((size_t)nt * nt, 0.0);
    for (int i = 0; i < nt - 1; i++)
        for (int j = i + 1; j < nt; j++) {
            double d = (double)w.tree_diff[(size_t)i * nt + j] / w.num_sites;
            if (c.jc) d = -0.75 * std::log(1.0 - (4.0 * d / 3.0));
            dist[(size_t)i * nt + j] = d;
            dist[(size_t)j * nt + i] = d;
        }
    Nj t(nt);
    t.join(dist);
    const int start = t.nd[t.nodep[0]].back;
    o.t("\t");
    t.print(o, start, start, c.refid ? c.refid : "", c.sample_names);
}

}  // namespace

void format_window(std::string &out, const pbg_cmd &c, int n, int np, uint32_t flag, const WindowHost &w) {
    W o{out};
    o.t(c.chr_name);
    o.t("\t");
    o.i(w.beg + 1);
    o.t("\t");
    o.i(w.end + 1);
    o.t("\t");
    o.i(w.num_sites);
    const bool ok = w.num_sites >= c.min_sites;
    switch (c.cmd) {
        case PBG_CMD_NUCDIV:  // print_nucdiv pop_nucdiv.cpp:258-289
            for (int i = 0; i < np; i++) {
                o.t("\tpi[" + pn(c, i) + "]:\t");
                if (ok) o.f(w.pi[i]); else o.na();
            }
            for (int i = 0; i < np - 1; i++)
                for (int j = i + 1; j < np; j++) {
                    o.t("\tdxy[" + pn(c, i) + "-" + pn(c, j) + "]:\t");
                    if (ok) o.f(w.dxy[i * np + (j - (i + 1))]); else o.na();
                }
            // --snn: per group (all populations as "*" first, with three or more; then every pair) Hudson's
            // Snn and its permutation p-value (ge + 1) / (PERMS + 1), after the reference's columns.  NA for
            // a window without a segregating site, the p-value also with no permutations; -k does not
            // blank them
            if ((c.output & PBG_NUCDIV_SNN) && np > 1 && w.snn_val.size() == snn_groups(np).size() &&
                w.snn_ge.size() == w.snn_val.size()) {
                const int perms = PBG_NUCDIV_SNN_PERMS(c.output);
                const bool seg = w.segsites >= 1;
                size_t e = 0;
                auto group = [&](const std::string &names) {
                    o.t("\tsnn[" + names + "]:\t");
                    if (seg) o.f(w.snn_val[e]); else o.na();
                    o.t("\tpsnn[" + names + "]:\t");
                    if (seg && perms > 0) o.f((double)(w.snn_ge[e] + 1) / (double)(perms + 1)); else o.na();
                    ++e;
                };
                if (np >= 3) group("*");
                for (int i = 0; i < np - 1; i++)
                    for (int j = i + 1; j < np; j++) group(pn(c, i) + "," + pn(c, j));
            }
            break;
        case PBG_CMD_SFS:  // print_sfs pop_sfs.cpp:293-317 (NA only for NaN)
            for (int i = 0; i < np; i++) {
                o.t("\tD[" + pn(c, i) + "]:\t");
                if (std::isnan(w.td[i])) o.na(); else o.f(w.td[i]);
                o.t("\tH[" + pn(c, i) + "]:\t");
                if (std::isnan(w.fwh[i])) o.na(); else o.f(w.fwh[i]);
            }
            // --theta: the integers and theta_W calc_sfs computes but print_sfs never prints,
            // appended after the reference's columns so the default output is unchanged
            if ((c.output & 1) && (int)w.seg_pop.size() == np && (int)w.sfs_bins.size() == np)
                for (int i = 0; i < np; i++) {
                    o.t("\tS[" + pn(c, i) + "]:\t");
                    o.i(w.seg_pop[i]);
                    o.t("\tthetaW[" + pn(c, i) + "]:\t");
                    if (!std::isfinite(w.theta_w[i])) o.na(); else o.f(w.theta_w[i]);
                    o.t("\tsfs[" + pn(c, i) + "]:\t");
                    for (size_t j = 0; j < w.sfs_bins[i].size(); j++) {
                        if (j) o.t(",");
                        o.i(w.sfs_bins[i][j]);
                    }
                }
            // --joint: per pair i < j Hudson's Fst and the joint spectrum's (n_i+1)*(n_j+1) cells
            // in cell order, after the reference's columns and --theta's
            if ((c.output & 2) && np > 1 && w.jsfs_fst.size() == (size_t)np * (np - 1) / 2 && (int)w.pop_n.size() == np) {
                const std::vector<int32_t> &pop_n = w.pop_n;
                size_t p = 0, at = 0;
                for (int i = 0; i < np - 1; i++)
                    for (int j = i + 1; j < np; j++, p++) {
                        const size_t cells = (size_t)(pop_n[i] + 1) * (pop_n[j] + 1);
                        if (at + cells > w.jsfs_cells.size()) break;
                        o.t("\tfst[" + pn(c, i) + "," + pn(c, j) + "]:\t");
                        if (std::isnan(w.jsfs_fst[p])) o.na(); else o.f(w.jsfs_fst[p]);
                        o.t("\tjsfs[" + pn(c, i) + "," + pn(c, j) + "]:\t");
                        for (size_t k = 0; k < cells; k++) {
                            if (k) o.t(",");
                            o.i(w.jsfs_cells[at + k]);
                        }
                        at += cells;
                    }
            }
            // --dstat: per triple (i, j, k) D, f_d, f_dM and the six sums they are formed from, after
            // --joint's columns
            if ((c.output & 4) && np > 2) {
                const std::vector<pbg_triple> tr = dstat_triples(np);
                if (w.dstat_d.size() == tr.size() && w.dstat_fd.size() == tr.size() && w.dstat_fdm.size() == tr.size() &&
                    w.dstat_sums.size() == tr.size() * 6)
                    for (size_t t = 0; t < tr.size(); t++) {
                        const std::string lab = "[" + pn(c, tr[t].p1) + "," + pn(c, tr[t].p2) + "," + pn(c, tr[t].p3) + "]:\t";
                        const std::pair<const char *, double> val[3] = {
                            {"\tD", w.dstat_d[t]}, {"\tfd", w.dstat_fd[t]}, {"\tfdM", w.dstat_fdm[t]}};
                        for (const auto &v : val) {
                            o.t(v.first + lab);
                            if (std::isnan(v.second)) o.na(); else o.f(v.second);
                        }
                        o.t("\tdsum" + lab);
                        for (int k = 0; k < 6; k++) {
                            if (k) o.t(",");
                            o.i(w.dstat_sums[t * 6 + k]);
                        }
                    }
            }
            break;
        case PBG_CMD_LD: {  // print_ld pop_ld.cpp:650-712
            const int ldo = c.output & 3;   // -o; bit 2 is --rmin
            for (int i = 0; i < np; i++) {
                o.t("\tS[" + pn(c, i) + "]:\t");
                o.i(w.ld_snps[i]);
                const bool sok = w.ld_snps[i] >= c.min_snps;
                if (ldo == 1) {
                    o.t("\tomax[" + pn(c, i) + "]:\t");
                    if (sok) o.f(w.ld_val[i]); else o.na();
                } else if (ldo == 2) {
                    o.t("\tB[" + pn(c, i) + "]:\t");
                    if (sok) o.f(w.ld_val[i]); else o.na();
                    o.t("\tQ[" + pn(c, i) + "]:\t");
                    if (sok) o.f(w.ld_q[i]); else o.na();
                } else {
                    o.t("\tZns[" + pn(c, i) + "]:\t");
                    if (sok) o.f(w.ld_val[i]); else o.na();
                }
            }
            // --decay: per population the bins' mean r^2 and pair counts, appended after the
            // reference's columns (the default output is unchanged); not subject to -n
            if (ldo == 0 && c.decay_bin > 0 && c.decay_bins > 0 &&
                w.decay_pairs.size() == (size_t)np * c.decay_bins && w.decay_sum.size() == w.decay_pairs.size())
                for (int i = 0; i < np; i++) {
                    const size_t b0 = (size_t)i * c.decay_bins;
                    o.t("\tdecay[" + pn(c, i) + "]:\t");
                    for (int k = 0; k < c.decay_bins; k++) {
                        if (k) o.t(",");
                        if (w.decay_pairs[b0 + k] == 0) o.t("NA");
                        else o.f(w.decay_sum[b0 + k] / (double)w.decay_pairs[b0 + k]);
                    }
                    o.t("\tpairs[" + pn(c, i) + "]:\t");
                    for (int k = 0; k < c.decay_bins; k++) {
                        if (k) o.t(",");
                        o.i(w.decay_pairs[b0 + k]);
                    }
                }
            // --rmin: per population Hudson and Kaplan's Rm and its intervals as left-right contig
            // positions, after the reference's columns and --decay's (any -o); not subject to -n
            if ((c.output & PBG_LD_RMIN) && (int)w.rmin_n.size() == np && w.rmin_cuts.size() == (size_t)np * w.rmin_stride * 2)
                for (int i = 0; i < np; i++) {
                    o.t("\tRmin[" + pn(c, i) + "]:\t");
                    o.i(w.rmin_n[i]);
                    o.t("\trint[" + pn(c, i) + "]:\t");
                    if (w.rmin_n[i] <= 0) o.t("NA");
                    for (int k = 0; k < w.rmin_n[i] && k < w.rmin_stride; k++) {
                        const size_t at = ((size_t)i * w.rmin_stride + k) * 2;
                        if (k) o.t(",");
                        o.i(w.rmin_cuts[at] + 1);
                        o.t("-");
                        o.i(w.rmin_cuts[at + 1] + 1);
                    }
                }
            break;
        }
        case PBG_CMD_DIVERGE:  // print_diverge pop_diverge.cpp:496-574
            if (c.output == 0) {
                for (int i = 0; i < n; i++) {
                    o.t(std::string("\td[") + c.sample_names[i] + "]:\t");
                    if (ok) o.f(w.div_ind[i]); else o.na();
                }
            } else {
                for (int i = 0; i < np; i++) {
                    const std::string p = pn(c, i);
                    if (ok) {
                        o.t("\tFixed[" + p + "]:\t");
                        o.i(w.div_fixed[i]);
                        o.t("\tSeg[" + p + "]:\t");
                        o.i(w.div_seg[i]);
                        o.t("\td[" + p + "]:\t");
                        o.f(w.div_pop[i]);
                    } else {
                        o.t("\tFixed[" + p + "]:\t");
                        o.na();
                        o.t("\tSeg[" + p + "]:\t");
                        o.na();
                        o.t("\td[" + p + "]:\t");
                        o.na();
                    }
                }
            }
            (void)flag;
            break;
        case PBG_CMD_HAPLO: {  // print_haplo pop_haplo.cpp:365-442
            const int ho = c.output & 3;   // -o; bit 2 is --nsl, bit 3 --xpnsl
            if (ho == 0) {
                for (int i = 0; i < np; i++) {
                    const std::string p = pn(c, i);
                    o.t("\tK[" + p + "]:\t");
                    if (ok) o.i(w.nhaps[i]); else o.na();
                    o.t("\tKdiv[" + p + "]:\t");
                    if (ok) o.f(w.hap_val[i]); else o.na();
                }
            } else if (ho == 1) {
                for (int i = 0; i < np; i++) {
                    o.t("\tEHHS[" + pn(c, i) + "]:\t");
                    if (ok && !std::isnan(w.hap_val[i])) o.f(w.hap_val[i]); else o.na();
                }
            } else {
                for (int i = 0; i < np; i++) {
                    o.t("\tpi[" + pn(c, i) + "]:\t");
                    if (ok) o.f(w.hap_val[i]); else o.na();
                }
                for (int i = 0; i < np - 1; i++)
                    for (int j = i + 1; j < np; j++) {
                        const std::string pp = pn(c, i) + "-" + pn(c, j);
                        const int k = i * np + (j - (i + 1));
                        o.t("\tdxy[" + pp + "]:\t");
                        if (ok) o.f(w.hap_dxy[k]); else o.na();
                        o.t("\tmin[" + pp + "]:\t");
                        if (ok) o.i(w.hap_min[k]); else o.na();
                    }
            }
            // --hfs: per population Garud's H statistics, the haplotype diversity and the class sizes,
            // after the reference's columns (the default output is unchanged); not subject to -k
            if (c.hfs && w.hfs_h.size() == (size_t)np * 5 && (int)w.hfs_k.size() == np &&
                w.hfs_counts.size() == (size_t)np * w.hfs_stride)
                for (int i = 0; i < np; i++) {
                    const std::string lab = "[" + pn(c, i) + "]:\t";
                    static const char *const nm[5] = {"\tH1", "\tH12", "\tH123", "\tH2H1", "\tHd"};
                    for (int k = 0; k < 5; k++) {
                        o.t(nm[k] + lab);
                        if (std::isnan(w.hfs_h[(size_t)i * 5 + k])) o.na(); else o.f(w.hfs_h[(size_t)i * 5 + k]);
                    }
                    o.t("\thfs" + lab);
                    for (int k = 0; k < w.hfs_k[i] && k < w.hfs_stride; k++) {
                        if (k) o.t(",");
                        o.i(w.hfs_counts[(size_t)i * w.hfs_stride + k]);
                    }
                }
            // --nsl: per population the variable sites as pos:m:value:c -- the 1-based contig position,
            // the derived count, the unstandardised nSL log((sl0 / P0) / (sl1 / P1)) (NA when a class
            // has no pair) and the number of tracts the window cut short -- after the reference's
            // columns and --hfs's (any -o); not subject to -k
            if ((c.output & PBG_HAPLO_NSL) && (int)w.pop_n.size() == np && w.nsl.holds(np, 1))
                for (int i = 0; i < np; i++) {
                    o.t("\tnsl[" + pn(c, i) + "]:\t");
                    if (w.nsl.n[i] <= 0) o.t("NA");
                    for (int k = 0; k < w.nsl.n[i] && k < w.nsl.stride; k++) {
                        const size_t at = (size_t)i * w.nsl.stride + k;
                        const long long m = w.nsl.m[at], z = w.pop_n[i] - m, p0 = z * (z - 1) / 2, p1 = m * (m - 1) / 2;
                        if (k) o.t(",");
                        o.i(w.nsl.pos[at] + 1);
                        o.t(":");
                        o.i(m);
                        o.t(":");
                        if (p0 == 0 || p1 == 0) o.t("NA");
                        else o.f(std::log(((double)w.nsl.sl[2 * at] / (double)p0) / ((double)w.nsl.sl[2 * at + 1] / (double)p1)));
                        o.t(":");
                        o.i((long long)w.nsl.cens[2 * at] + w.nsl.cens[2 * at + 1]);
                    }
                }
            // --xpnsl: per population pair (i < j) the pooled sites as pos:mI:mJ:value:c -- the 1-based contig
            // position, the two derived counts, the unstandardised XP-nSL log((sl_i / C_i) / (sl_j / C_j))
            // with C = n (n - 1) / 2 (NA when a side has no pair, or two samples that differ) and the number
            // of tracts the window cut short, both sides together -- after --nsl's columns; not subject to -k
            const size_t xp = (size_t)np * (np - 1) / 2;
            if ((c.output & PBG_HAPLO_XPNSL) && xp > 0 && (int)w.pop_n.size() == np && w.xpnsl.holds(xp, 2)) {
                size_t p = 0;
                for (int i = 0; i < np; i++)
                    for (int j = i + 1; j < np; j++, p++) {
                        o.t("\txpnsl[" + pn(c, i) + "," + pn(c, j) + "]:\t");
                        if (w.xpnsl.n[p] <= 0) o.t("NA");
                        const long long c0 = (long long)w.pop_n[i] * (w.pop_n[i] - 1) / 2, c1 = (long long)w.pop_n[j] * (w.pop_n[j] - 1) / 2;
                        for (int k = 0; k < w.xpnsl.n[p] && k < w.xpnsl.stride; k++) {
                            const size_t at = p * w.xpnsl.stride + k;
                            const long long s0 = w.xpnsl.sl[2 * at], s1 = w.xpnsl.sl[2 * at + 1];
                            if (k) o.t(",");
                            o.i(w.xpnsl.pos[at] + 1);
                            o.t(":");
                            o.i(w.xpnsl.m[2 * at]);
                            o.t(":");
                            o.i(w.xpnsl.m[2 * at + 1]);
                            o.t(":");
                            if (c0 == 0 || c1 == 0 || s0 == 0 || s1 == 0) o.t("NA");
                            else o.f(std::log(((double)s0 / (double)c0) / ((double)s1 / (double)c1)));
                            o.t(":");
                            o.i((long long)w.xpnsl.cens[2 * at] + w.xpnsl.cens[2 * at + 1]);
                        }
                    }
            }
            break;
        }
        case PBG_CMD_TREE:
            format_nj(o, c, n, w);
            break;
        default:
            break;
    }
    out += "\n";
}

namespace {
// "=ACMGRSVTWYHKDBN"[bam_nt16_table[c]] (popbam.cpp:13-31) for letters
char nt16_letter(unsigned char c) {
    static const char rev[] = "=ACMGRSVTWYHKDBN";
    static const char *letters = "ACMGRSVTWYHKDBN";
    unsigned char u = (c >= 'a' && c <= 'z') ? (unsigned char)(c - 32) : c;
    if (u == '=') return '=';
    for (int i = 0; letters[i]; ++i)
        if (letters[i] == (char)u) return rev[i + 1];
    return 'N';
}
const char kIupac[16] = {'A', 'M', 'R', 'W', 'N', 'C', 'S', 'Y', 'N', 'N', 'G', 'K', 'N', 'N', 'N', 'T'};
}  // namespace

void format_snp_site(std::string &out, const pbg_cmd &c, int n, int32_t pos, unsigned char refc, const uint64_t *cb) {
    W o{out};
    o.t(c.chr_name);
    o.t("\t");
    o.i((long long)pos + 1);
    o.t("\t");
    out += nt16_letter(refc);
    for (int j = 0; j < n; j++) {
        const unsigned g = (unsigned)(cb[j] >> 8) & 0xff;
        // genotype bytes >= 16 only arise from segbase's borrow; the reference then reads
        // iupac[] out of bounds (undefined); we print 'N'
        out += "\t";
        out += g < 16 ? nt16_letter((unsigned char)kIupac[g]) : 'N';
        o.t("\t");
        o.i((long long)((cb[j] >> 32) & 0xffff));
        o.t("\t");
        o.i((long long)((cb[j] >> 48) & 0xffff));
        o.t("\t");
        o.i((long long)((cb[j] >> 16) & 0xffff));
    }
    out += "\n";
}

// snp -o 1: print_sweep (pop_snp.cpp:243-268).  At a counted site every sample passes
// qfilter, so the reference's pop_sample_mask (sample_cov & pop_mask) is pop_mask.
void format_sweep_site(std::string &out, const pbg_cmd &c, int np, const mask128 *pop_mask, uint32_t flag,
                       int32_t pos, mask128 types) {
    W o{out};
    o.t(c.chr_name);
    o.t("\t");
    o.i((long long)pos + 1);
    for (int j = 0; j < np; j++) {
        const mask128 pt = types & pop_mask[j];
        const unsigned pop_n = (unsigned)popcount128(pop_mask[j]);
        const bool flip = (flag & PBG_F_OUTGROUP) && ((types >> c.outidx) & 1);
        const unsigned freq = (unsigned short)(flip ? pop_n - (unsigned)popcount128(pt) : (unsigned)popcount128(pt));
        o.t("\t");
        o.i(freq);
        o.t("\t");
        o.i(pop_n);
    }
    out += "\n";
}

// snp -o 2: print_ms_header (pop_snp.cpp:305-317), once before the first window
void format_ms_header(std::string &out, int n, int np, const int32_t *pop_n, long nwindows) {
    W o{out};
    o.t("ms ");
    o.i(n);
    o.t(" ");
    o.i(nwindows);
    if (np > 1) {
        o.t(" -t 5.0 -I ");
        o.i(np);
        o.t(" ");
        for (int i = 0; i < np; i++) {
            o.i(pop_n[i]);
            o.t(" ");
        }
    } else {
        o.t(" -t 5.0 ");
    }
    out += "\n1350154902\n\n";
}

// snp -o 2: print_ms (pop_snp.cpp:270-303) for one window [wbeg, wend): positions relative to
// the window as std::setprecision(8) (printf "%.8g"), then one 0/1 string per sample, the
// derived bit flipped where the outgroup carries it.
void format_ms_window(std::string &out, int n, uint32_t flag, int outidx, int32_t wbeg, int32_t wend,
                      const std::vector<int32_t> &pos, const std::vector<mask128> &types) {
    W o{out};
    const size_t S = pos.size();
    o.t("//\nsegsites: ");
    o.i((long long)S);
    o.t("\npositions: ");
    for (size_t i = 0; i < S; i++) {
        char b[64];
        std::snprintf(b, sizeof b, "%.8g ", (double)(unsigned)(pos[i] - wbeg) / (double)(wend - wbeg));
        out += b;
    }
    out += "\n";
    for (int i = 0; i < n; i++) {
        for (size_t j = 0; j < S; j++) {
            const bool d = (types[j] >> i) & 1;
            const bool flip = (flag & PBG_F_OUTGROUP) && ((types[j] >> outidx) & 1);
            out += d != flip ? '1' : '0';
        }
        out += "\n";
    }
    out += "\n";
}

}  // namespace pbg
