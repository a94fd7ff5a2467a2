"""LD decay beside ZnS on one resident batch: `python tools/decay_time.py [--sites 50000000]
[--samples 12] [--pops 2] [--window 10000] [--reps 25]`.

The BASELINE configs[2] shape by default: 50 Msites x 12 samples, 10 kb reference windows, rows
from one HotPath.call.  Times, warm, with device events around each call (median of --reps, at
least 20): pbg_window_ld_decay at (bin_bp, n_bins) = (100, 100) and (20000, 1), and
pbg_window_stats(PBG_S_ZNS) on the same rows in the same process -- the yardstick: it visits the
same pairs.  A (1, 1) call shows the gather's share.  The calls are timed in turn, rep by rep.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

from popbam_amd import _lib, workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=12)
ap.add_argument("--pops", type=int, default=2)
ap.add_argument("--sites", type=int, default=50_000_000)
ap.add_argument("--window", type=int, default=10_000)
ap.add_argument("--depth", type=int, default=10)
ap.add_argument("--reps", type=int, default=25)
ap.add_argument("--seed", type=lambda s: int(s, 0), default=0xC0FFEE02)
a = ap.parse_args()
if a.reps < 20:
    ap.error("--reps must be at least 20")
assert torch.cuda.is_available(), "decay_time.py needs a GPU"
sites = a.sites // 64 * 64
ctx = _lib.Context(workload.default_params(a.samples, a.pops), 0)
syn = workload.SynthPileup(ctx, sites, a.depth, a.seed)
wins = workload.reference_windows(0, sites, a.window)
hp = workload.HotPath(ctx, syn, wins, _lib.PBG_S_ZNS)
hp.call()
ctx.sync_check()
st = torch.cuda.current_stream()
cases = {"decay_100x100": workload.LdDecay(ctx, hp.n_win, 100, 100),
         "decay_20000x1": workload.LdDecay(ctx, hp.n_win, 20000, 1),
         # one bin of one base: the gather and an almost empty walk (what the kernel costs before it bins)
         "decay_1x1": workload.LdDecay(ctx, hp.n_win, 1, 1)}
runs = {"zns": hp.window_stats}
for nm, d in cases.items():
    runs[nm] = (lambda d=d: d(hp.rows, hp.wins, sites))
for f in runs.values():   # warm: plans, workspace, code objects
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
d = cases["decay_100x100"]
out = {"sites": sites, "samples": a.samples, "pops": a.pops, "window": a.window, "windows": hp.n_win, "reps": a.reps,
       "variable_sites": int(d.n_var.sum().item()), "pairs_100x100": int(d.pairs.sum().item()),
       "pairs_20000x1": int(cases["decay_20000x1"].pairs.sum().item()),
       "lib": ctx.lib.pbg_build_info().decode()}
for nm, v in ms.items():
    out[nm + "_ms_median"] = round(statistics.median(v), 4)
    out[nm + "_ms_min"] = round(min(v), 4)
    out[nm + "_ms_max"] = round(max(v), 4)
print(json.dumps(out))
