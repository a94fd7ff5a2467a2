"""The haplotype-spectrum pass beside the joint-spectrum pass on one resident batch:
`python tools/hfs_time.py [--sites 50000000] [--samples 12] [--pops 2] [--window 10000] [--reps 25]
[--jsfs-tree DIR] [--out FILE]`.

The BASELINE configs[2] shape by default: 50 Msites x 12 samples x 2 populations, 10 kb reference
windows, rows from one HotPath.call.  Times, warm, with device events around each call (median of
--reps, at least 20): pbg_window_hfs (all five outputs; and once more with k, sums and h alone,
which skips the per-sample and per-slot stores) and pbg_window_jsfs (all three) on the same rows and
windows -- the yardstick: the existing kernel that streams the same rows.  The calls are timed in
turn, rep by rep.

--jsfs-tree DIR takes the yardstick from a built checkout of another commit (the parent's, which has
no pbg_window_hfs): a fresh child process runs this script with --only-jsfs --tree DIR, so that it
imports DIR's popbam_amd package and library, on the same seed and shape, before this process
touches the GPU.  Prints one JSON line (and writes it to --out): both times and hfs / jsfs."""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=12)
ap.add_argument("--pops", type=int, default=2)
ap.add_argument("--sites", type=int, default=50_000_000)
ap.add_argument("--window", type=int, default=10_000)
ap.add_argument("--depth", type=int, default=10)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0FFEE02)
ap.add_argument("--jsfs-tree", default="")
ap.add_argument("--only-jsfs", action="store_true")
ap.add_argument("--tree", default=REPO, help="the checkout whose popbam_amd package is imported")
ap.add_argument("--out", default="")
a = ap.parse_args()
if a.reps < 20:
    ap.error("--reps must be at least 20")
if a.pops < 2:
    ap.error("--pops must be at least 2 (the yardstick needs a population pair)")

parent = None
if a.jsfs_tree:
    argv = [sys.executable, os.path.abspath(__file__), "--only-jsfs", "--tree", os.path.abspath(a.jsfs_tree)]
    for k in ("samples", "pops", "sites", "window", "depth", "reps", "seed"):
        argv += ["--" + k, str(getattr(a, k))]
    env = {k: v for k, v in os.environ.items() if k != "POPBAM_GPU_LIB"}
    r = subprocess.run(argv, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("the --jsfs-tree run failed:\n" + r.stderr[-2000:])
    parent = json.loads(r.stdout.strip().splitlines()[-1])

sys.path.insert(0, os.path.abspath(a.tree))
import torch  # noqa: E402

from popbam_amd import _lib, workload  # noqa: E402

assert torch.cuda.is_available(), "hfs_time.py needs a GPU"
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
j = workload.JointSfs(ctx, hp.n_win)
runs = {"jsfs": lambda: j(hp.rows, hp.wins, sites)}
h = None
if not a.only_jsfs:
    h = workload.Hfs(ctx, hp.n_win)
    runs["hfs"] = lambda: h(hp.rows, hp.wins, sites)
    hs = workload.Hfs(ctx, hp.n_win)   # per population only: without the counts and the class labels
    hs.out.counts = hs.out.cls = None
    runs["hfs_pop"] = lambda: hs(hp.rows, hp.wins, sites)
for f in runs.values():   # warm: tables, code objects
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
out = {"sites": sites, "samples": a.samples, "pops": a.pops, "window": a.window, "windows": hp.n_win, "reps": a.reps,
       "segsites": int(hp.out.t["segsites"].sum().item()), "lib": ctx.lib.pbg_build_info().decode(),
       "tree": "this" if os.path.abspath(a.tree) == REPO else "other"}
for nm, v in ms.items():
    out[nm + "_ms_median"] = round(statistics.median(v), 4)
    out[nm + "_ms_min"] = round(min(v), 4)
    out[nm + "_ms_max"] = round(max(v), 4)
if h is not None:
    out["classes"] = int(h.k.sum().item())
    base = out["jsfs_ms_median"]
    if parent is not None:
        assert parent["segsites"] == out["segsites"], "the --jsfs-tree run saw other rows"
        out["jsfs_parent_ms_median"], out["jsfs_parent_ms_min"], out["jsfs_parent_ms_max"] = (
            parent["jsfs_ms_median"], parent["jsfs_ms_min"], parent["jsfs_ms_max"])
        base = parent["jsfs_ms_median"]
    out["hfs_over_jsfs"] = round(out["hfs_ms_median"] / base, 4)
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
