"""The window passes on one resident batch, for one or more built checkouts:
`python tools/window_time.py [--passes sfs,decay,jsfs,dstat,hfs,rmin,nsl,xpnsl,snn] [--tree DIR]... [--sites 50000000]
[--samples 12] [--pops 2] [--window 10000] [--depth 10] [--reps 25] [--seed 0xC0FFEE02] [--out FILE]`.

The BASELINE configs[2] shape by default: 50 Msites x 12 samples x 2 populations, 10 kb reference
windows, rows from one HotPath.call.  Each pass is timed warm, with device events around each call
(median, min and max of --reps, at least 20), the calls in turn, rep by rep, on the same rows and
windows:
  sfs    pbg_window_stats(PBG_S_SFS)
  decay  pbg_window_ld_decay at (bin_bp, n_bins) = (100, 100), (20000, 1) and (1, 1): decay_100x100,
         decay_20000x1, decay_1x1 (the last is the gather and an almost empty walk)
  jsfs   pbg_window_jsfs, all three outputs
  dstat  pbg_window_dstat over all triples (i, j, k), i < j, k neither: all four outputs, and
         dstat_sums without the last stage's divisions.  Needs --pops 3 or more; skipped below that.
  hfs    pbg_window_hfs: all five outputs, and hfs_pop with k, sums and h alone
  rmin   pbg_window_rmin with rmin and n_var alone, and rmin_cuts with max_cuts = 64 and all three
  nsl    pbg_window_nsl count-only (max_sites = 0) as nsl_nvar, and nsl, the full call with all five
         outputs and max_sites = the largest count nsl_nvar found
  xpnsl  pbg_window_xpnsl count-only as xpnsl_nvar, and xpnsl, the full call with all five outputs and
         max_sites = the largest count xpnsl_nvar found.  Needs --pops 2 or more; skipped below that.
  snn    pbg_window_snn with n_groups = 0 and diff alone as pairdiff, and snn_1000: all populations together
         (with three or more) and every pair, 1,000 permutations, all four outputs; its line also carries
         snn_1000_ns_per_perm, the time per (window, group, permutation).  snn_1000 needs --pops 2 or more.
A tree without one of the calls cannot run that pass; rmin, nsl, xpnsl and snn alone are skipped there (and
named in `skipped`): rmin's yardstick is the decay_1x1 of the tree before it, nsl's is that tree's rmin,
and with two trees of which the first has no nsl the comparison sets nsl_nvar against the first
tree's rmin and gives nsl's ratio to it (when both trees have nsl, it is compared pass against pass
like every other); likewise the yardsticks of xpnsl are the nsl_nvar and nsl of a first tree without xpnsl, and the
comparison gives the ratios;
pairdiff's yardstick is the first tree's sfs, which streams the same rows; snn_1000 has no predecessor.

Every --tree (default: this checkout) is measured in a fresh child process that imports that tree's
popbam_amd package and library; this process never touches the GPU.  Two or more trees are measured
in turn, twice over (A, B, A, B), so that each tree's own run-to-run difference is seen beside the
difference between the trees.  Prints one JSON line per child (and writes them to --out), each with
`segsites` and pbg_build_info(); trees whose `segsites` differ saw other rows and are not compared.
With two trees a last line compares the second with the first, pass by pass: the mean of each tree's
two medians, and `ok` when the second is not above the first by more than the larger of the first
tree's own difference and 2 % (profiles/INDEX.md: the largest difference recorded between the same
kernel's runs on two builds)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("sfs", "decay", "jsfs", "dstat", "hfs", "rmin", "nsl", "xpnsl", "snn")
SHAPE = ("samples", "pops", "sites", "window", "depth", "reps", "seed")


def child(a, passes):
    sys.path.insert(0, a.tree[0])
    import torch
    from popbam_amd import _lib, workload

    assert torch.cuda.is_available(), "window_time.py needs a GPU"
    sites = a.sites // 64 * 64
    ctx = _lib.Context(workload.default_params(a.samples, a.pops), 0)
    syn = workload.SynthPileup(ctx, sites, a.depth, a.seed)
    wins = workload.reference_windows(0, sites, a.window)
    hp = workload.HotPath(ctx, syn, wins, _lib.PBG_S_SFS)
    hp.call()
    ctx.sync_check()
    hp.window_stats()   # segsites: the rows every pass below works on
    ctx.sync_check()
    st = torch.cuda.current_stream()
    runs, skipped = {}, []

    def on_rows(x):
        return lambda: x(hp.rows, hp.wins, sites)

    if "sfs" in passes:
        runs["sfs"] = hp.window_stats
    if "decay" in passes:
        for bin_bp, n_bins in ((100, 100), (20000, 1), (1, 1)):
            runs[f"decay_{bin_bp}x{n_bins}"] = on_rows(workload.LdDecay(ctx, hp.n_win, bin_bp, n_bins))
    if "jsfs" in passes:
        runs["jsfs"] = on_rows(workload.JointSfs(ctx, hp.n_win))
    if "dstat" in passes and a.pops < 3:
        skipped.append("dstat")
    elif "dstat" in passes:
        triples = [(i, j, k) for i in range(a.pops) for j in range(i + 1, a.pops) for k in range(a.pops) if k not in (i, j)]
        runs["dstat"] = on_rows(workload.DStat(ctx, hp.n_win, triples))
        ds = workload.DStat(ctx, hp.n_win, triples)
        ds.out.d = ds.out.fd = ds.out.fdm = None
        runs["dstat_sums"] = on_rows(ds)
    if "hfs" in passes:
        runs["hfs"] = on_rows(workload.Hfs(ctx, hp.n_win))
        hs = workload.Hfs(ctx, hp.n_win)
        hs.out.counts = hs.out.cls = None
        runs["hfs_pop"] = on_rows(hs)
    if "rmin" in passes and not hasattr(workload, "Rmin"):
        skipped.append("rmin")   # a tree from before the call: its decay_1x1 is the yardstick
    elif "rmin" in passes:
        runs["rmin"] = on_rows(workload.Rmin(ctx, hp.n_win))
        runs["rmin_cuts"] = on_rows(workload.Rmin(ctx, hp.n_win, 1, 64))
    extra = {}
    if "nsl" in passes and not hasattr(workload, "Nsl"):
        skipped.append("nsl")   # a tree from before the call: its rmin is the yardstick
    elif "nsl" in passes:
        cnt = workload.Nsl(ctx, hp.n_win)
        runs["nsl_nvar"] = on_rows(cnt)
        cnt(hp.rows, hp.wins, sites)
        ctx.sync_check()
        extra["nsl_max_sites"] = int(cnt.n_var.max().item())
        extra["nsl_sites"] = int(cnt.n_var.sum().item())
        if extra["nsl_max_sites"] > 0:
            runs["nsl"] = on_rows(workload.Nsl(ctx, hp.n_win, extra["nsl_max_sites"]))
    if "xpnsl" in passes and (not hasattr(workload, "Xpnsl") or a.pops < 2):
        skipped.append("xpnsl")   # a tree from before the call: its nsl is the yardstick
    elif "xpnsl" in passes:
        cnt = workload.Xpnsl(ctx, hp.n_win)
        runs["xpnsl_nvar"] = on_rows(cnt)
        cnt(hp.rows, hp.wins, sites)
        ctx.sync_check()
        extra["xpnsl_max_sites"] = int(cnt.n_var.max().item())
        extra["xpnsl_sites"] = int(cnt.n_var.sum().item())
        if extra["xpnsl_max_sites"] > 0:
            runs["xpnsl"] = on_rows(workload.Xpnsl(ctx, hp.n_win, extra["xpnsl_max_sites"]))
    if "snn" in passes and not hasattr(workload, "Snn"):
        skipped.append("snn")   # a tree from before the call: its sfs is pairdiff's yardstick
    elif "snn" in passes:
        pd = workload.Snn(ctx, hp.n_win)
        runs["pairdiff"] = on_rows(pd)
        groups = workload.Snn.default_groups(a.pops)
        if groups:
            runs["snn_1000"] = on_rows(workload.Snn(ctx, hp.n_win, groups, 1000))
            extra["snn_groups"] = len(groups)
            extra["snn_chunks"] = workload.Snn(ctx, hp.n_win, groups, 1000).chunks
    for f in runs.values():   # warm: plans, workspace, tables, code objects
        f()
        f()
    ctx.sync_check()
    ms = {nm: [] for nm in runs}
    for _ in range(a.reps):
        for nm, f in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            f()
            e1.record(st)
            e1.synchronize()
            ms[nm].append(e0.elapsed_time(e1))
    ctx.sync_check()
    out = {"tree": "this" if a.tree[0] == REPO else "other: " + os.path.basename(a.tree[0]), "sites": sites,
           "samples": a.samples, "pops": a.pops, "window": a.window, "windows": hp.n_win, "reps": a.reps,
           "segsites": int(hp.out.t["segsites"].sum().item()), "lib": ctx.lib.pbg_build_info().decode(),
           "skipped": skipped, **extra}
    for nm, v in ms.items():
        out[nm + "_ms_median"] = round(statistics.median(v), 4)
        out[nm + "_ms_min"] = round(min(v), 4)
        out[nm + "_ms_max"] = round(max(v), 4)
    if "snn_1000" in ms:
        out["snn_1000_ns_per_perm"] = round(statistics.median(ms["snn_1000"]) * 1e6 / (hp.n_win * extra["snn_groups"] * 1000), 3)
    print(json.dumps(out))


def compare(first, second):
    """The second tree against the first: {pass: {...}} from each tree's two result lines."""
    cmp = {}
    for key in first[0]:
        if not key.endswith("_ms_median"):
            continue
        a = [r[key] for r in first]
        base, new = statistics.mean(a), statistics.mean(r[key] for r in second)
        margin = max(max(a) - min(a), 0.02 * base)
        cmp[key[:-len("_ms_median")]] = {"first_ms": round(base, 4), "second_ms": round(new, 4), "margin_ms": round(margin, 4),
                                         "ok": new <= base + margin}
    if "rmin_ms_median" in first[0] and "nsl_nvar_ms_median" in second[0] and "nsl_nvar_ms_median" not in first[0]:
        # nsl against the rmin of a first tree that has no nsl of its own
        a = [r["rmin_ms_median"] for r in first]
        base = statistics.mean(a)
        margin = max(max(a) - min(a), 0.02 * base)
        for nm in ("nsl_nvar", "nsl"):
            if nm + "_ms_median" in second[0]:
                new = statistics.mean(r[nm + "_ms_median"] for r in second)
                cmp[nm] = {"first_rmin_ms": round(base, 4), "second_ms": round(new, 4), "ratio": round(new / base, 3)}
        cmp["nsl_nvar"].update(margin_ms=round(margin, 4), ok=cmp["nsl_nvar"]["second_ms"] <= base + margin)
    for nm, yard in (("xpnsl_nvar", "nsl_nvar"), ("xpnsl", "nsl")):   # xpnsl against the nsl of a first tree without xpnsl
        if yard + "_ms_median" in first[0] and nm + "_ms_median" in second[0] and nm + "_ms_median" not in first[0]:
            base = statistics.mean(r[yard + "_ms_median"] for r in first)
            new = statistics.mean(r[nm + "_ms_median"] for r in second)
            cmp[nm] = {f"first_{yard}_ms": round(base, 4), "second_ms": round(new, 4), "ratio": round(new / base, 3)}
    if "sfs_ms_median" in first[0] and "pairdiff_ms_median" in second[0]:   # pairdiff against the first tree's sfs
        base = statistics.mean(r["sfs_ms_median"] for r in first)
        new = statistics.mean(r["pairdiff_ms_median"] for r in second)
        cmp["pairdiff"] = {"first_sfs_ms": round(base, 4), "second_ms": round(new, 4), "ratio": round(new / base, 3)}
    if "snn_1000_ms_median" in second[0]:
        cmp["snn_1000"] = {"second_ms": round(statistics.mean(r["snn_1000_ms_median"] for r in second), 4),
                           "ns_per_perm": round(statistics.mean(r["snn_1000_ns_per_perm"] for r in second), 3)}
    return cmp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", default=",".join(PASSES))
    ap.add_argument("--tree", action="append", default=[], help="a built checkout; repeatable (default: this one)")
    ap.add_argument("--samples", type=int, default=12)
    ap.add_argument("--pops", type=int, default=2)
    ap.add_argument("--sites", type=int, default=50_000_000)
    ap.add_argument("--window", type=int, default=10_000)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0FFEE02)
    ap.add_argument("--out", default="")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    passes = [p for p in a.passes.split(",") if p]
    if not passes or set(passes) - set(PASSES):
        ap.error("--passes takes a subset of " + ",".join(PASSES))
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    if a.child:
        return child(a, passes)
    trees = [os.path.abspath(t) for t in a.tree] or [REPO]
    env = {k: v for k, v in os.environ.items() if k != "POPBAM_GPU_LIB"}
    results = []
    for tree in trees * (2 if len(trees) > 1 else 1):
        argv = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--passes", ",".join(passes)]
        for k in SHAPE:
            argv += ["--" + k, str(getattr(a, k))]
        r = subprocess.run(argv, env=env, capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the GPU after a failed run
            sys.exit(f"the run of {tree} failed ({r.returncode}):\n" + r.stderr[-2000:])
        results.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(results[-1]), flush=True)
    lines = [json.dumps(r) for r in results]
    if len({r["segsites"] for r in results}) > 1:
        sys.exit("the trees saw other rows (segsites differ): not comparable")
    if len(trees) == 2:
        lines.append(json.dumps({"compare": compare(results[0::2], results[1::2]), "first": results[0]["tree"],
                                 "second": results[1]["tree"]}))
        print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
