"""Helpers shared by the tests of the two tract calls (test_nsl.py, test_xpnsl.py, test_tract_edges.py):
bit arithmetic for the checkers, the called and the crafted inputs, the sized run, the body of the
determinism-and-interleaving test and the child process of the PBG_BOUNDS build.  The checkers
themselves (`ref_nsl`, `ref_xpnsl`, the `chain_*` functions, the hand-made windows) stay with their
tests."""
import json
import os
import subprocess
import sys
from functools import partial

import numpy as np

import harness
from window_helpers import _arrays, _blocks, mask_words, _wins_tensor

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")
SEED = 0x4A1   # test_rmin.py's: the same called rows
COUNTED, SEG = 2, 4   # harness flags bits
NAMES = ("n_var", "row", "m", "sl", "cens")


def local_bits(x, pm):
    """The bits of column x at the samples of mask pm, by ascending sample id."""
    out, s = [], 0
    while pm >> s:
        if (pm >> s) & 1:
            out.append((x >> s) & 1)
        s += 1
    return out


def row_ints(types):
    lo, hi = mask_words(types)
    return [int(a) | (int(b) << 64) for a, b in zip(lo.tolist(), hi.tolist())]


def _assert_same(got, want, what=""):
    for g, w, nm in zip(got, want, NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, nm, g.shape, w.shape, g.dtype, w.dtype)
        same = g == w
        assert same.all(), (what, nm, np.argwhere(~same)[:5].tolist(), g[~same][:5], w[~same][:5])


def _founder_cols(rng, V, n, founders, stretch):
    """Columns in which every sample copies one of a few founders, the copy changing every `stretch`
    sites: pairs on one founder agree for the whole stretch."""
    cols = []
    for k0 in range(0, V, stretch):
        src = rng.integers(0, founders, n)
        for _ in range(min(stretch, V - k0)):
            fb = rng.integers(0, 2, founders)
            cols.append([int(x) for x in fb[src]])
    return cols


# ---- GPU inputs --------------------------------------------------------------------------
N_SITES = 32_000
SHAPES = {   # name -> (samples, population masks): the shapes of test_rmin.py
    "n12p2": (12, _blocks([6, 6])),                                   # 2-byte rows
    "n24p3": (24, _blocks([8, 8, 8])),                                # 4-byte rows
    "n40p2i": (40, [sum(1 << s for s in range(0, 40, 2)), sum(1 << s for s in range(1, 40, 2))]),   # 8-byte rows
    "n96p4": (96, _blocks([24] * 4)),                                 # 16-byte rows, six pairs
    # population 0 straddles the words; 2,415 pairs, or 3,640 for 70 + 50: one wave per workgroup
    "n126p3": (126, _blocks([70, 50, 6])),
    "n14one": (14, [0b00000000111111, 0b00000001000000, 0b11111100000000]),   # a population of one; sample 7 in none
}
WIDE = ("n40p2i", "n96p4", "n126p3")   # windows of up to 3,000 rows, so that the checkers stay within seconds
_shapes = {}


def _params(n, masks, flag=0):
    from popbam_amd import workload
    params = workload.default_params(n, len(masks), flag=flag)
    for i, m in enumerate(masks):
        params.set_pop_mask(i, m)
        params.pop_n[i] = bin(m).count("1")
    return params


def _shape(name):
    """One called synthetic batch per shape, shared by the tests (read only)."""
    if name not in _shapes:
        import torch
        from popbam_amd import _lib, workload
        n, masks = SHAPES[name]
        params = _params(n, masks)
        ctx = _lib.Context(params, 0)
        syn = workload.SynthPileup(ctx, N_SITES, 10, SEED + n)
        hp = workload.HotPath(ctx, syn, [(0, N_SITES)], _lib.PBG_S_SFS)
        hp.call()
        ctx.sync_check()
        torch.cuda.synchronize()
        types, flags = harness.rows_to_sites(hp.rows.cpu().numpy(), ctx.row_bytes, N_SITES, n)
        _shapes[name] = (ctx, params, hp.rows, types, flags)
    return _shapes[name]


def _windows(n_sites, whole):
    """Windows from 3 rows up: overlapping, empty, beg == end, beg > end; the whole batch when asked."""
    rng = np.random.default_rng(7)
    wins = [(0, n_sites) if whole else (0, 3_000), (0, 2_000), (9_999, 12_001), (5, 5), (0, 1), (9, 4)]
    for ln in (3, 10, 30, 60, 100, 150, 300, 1000, 3000):
        for s in rng.integers(0, n_sites - ln, 2):
            wins.append((int(s), int(s) + ln))
    return wins


def _run_tract(call, ctx, rows, n_rows, wins, max_sites=0):
    """workload.<call> (Nsl or Xpnsl) over the windows -> its five arrays."""
    from popbam_amd import workload
    j = getattr(workload, call)(ctx, len(wins), max_sites)
    j(rows, _wins_tensor(wins), n_rows)
    ctx.sync_check()
    return _arrays(j, NAMES)


_run_nsl, _run_xpnsl = partial(_run_tract, "Nsl"), partial(_run_tract, "Xpnsl")


def _run_sized(ctx, rows, n_rows, wins, run):
    """The way the command line sizes the per-site arrays: the counts first, then max_sites = the largest."""
    got = run(ctx, rows, n_rows, wins, 0)
    n_var = got[0]
    assert got[1].shape == (len(wins), n_var.shape[1], 0) and got[3].shape == (len(wins), n_var.shape[1], 0, 2)
    ms = int(n_var.max()) if n_var.size else 0
    if ms == 0:
        return got, 0
    got = run(ctx, rows, n_rows, wins, ms)
    assert np.array_equal(got[0], n_var)
    return got, ms


def _founder_types(rng, L, n, founders):
    """Rows in which every sample copies one of a few founders (the copy changes every 64 rows): samples
    on one founder are identical for the whole stretch (test_rmin.py's)."""
    out = np.zeros((L, 2), np.uint64)
    for r0 in range(0, L, 64):
        src = rng.integers(0, founders, n)
        fb = rng.integers(0, 2, (min(64, L - r0), founders))
        sb = fb[:, src]   # [rows, n]
        for s in range(n):
            out[r0:r0 + len(sb), s >> 6] |= sb[:, s].astype(np.uint64) << np.uint64(s & 63)
    return out if n > 64 else out[:, 0].copy()


def _crafted(n, masks, types, flags):
    """A context with the given population masks and device rows packed from (types, flags)."""
    import torch
    from popbam_amd import _lib
    params = _params(n, masks)
    ctx = _lib.Context(params, 0)
    rows = torch.from_numpy(harness.rows_from_oracle(types, flags, ctx.row_bytes).copy()).cuda()
    return ctx, params, rows


def _padded(rows):
    """The rows in a larger buffer of 0xFF bytes."""
    import torch
    big = torch.full((rows.numel() + 4096,), 0xFF, dtype=torch.uint8, device="cuda")
    big[:rows.numel()] = rows
    return big


# ---- the determinism-and-interleaving test -------------------------------------------------
def _interleaving(key, sized, others, order):
    """Statistics, the calls of `order`, statistics, with the same pointers on one context and stream:
    each equals its own stand-alone run on a fresh context byte for byte, and so do the runs of `key`
    with one member NULL.  `sized`: the tract calls (workload class names; their keys are the lower-case
    names), run at max_sites = their largest count; others(wins): {key: (context -> call, array names)}."""
    from popbam_amd import _lib, workload
    n, npops, L = 12, 3, 64 * 500
    wins = [(0, 6000)] + workload.reference_windows(0, L, 10_000) + [(s, s + 400) for s in range(0, 8000, 200)]

    def fresh():
        ctx = _lib.Context(workload.default_params(n, npops), 0)
        syn = workload.SynthPileup(ctx, L, 10, SEED)
        hp = workload.HotPath(ctx, syn, wins, _lib.PBG_S_ZNS)
        hp.call()
        ctx.sync_check()
        return ctx, hp

    def zns(hp):
        hp.out.t["ld_val"].fill_(-1.0)
        hp.out.t["ld_snps"].fill_(-1)
        hp.window_stats()

    def zns_out(hp):
        return hp.out.t["ld_snps"].cpu().numpy().tobytes(), hp.out.t["ld_val"].cpu().numpy().tobytes()

    ctx, hp = fresh()
    cnt = [getattr(workload, c)(ctx, len(wins))(hp.rows, hp.wins, L) for c in sized]
    ctx.sync_check()
    ms = {c: int(x.n_var.max().item()) for c, x in zip(sized, cnt)}
    assert min(ms.values()) > 20
    ctx.close()
    make = dict(others(wins))
    for c in sized:
        make[c.lower()] = (lambda ctx, c=c: getattr(workload, c)(ctx, len(wins), ms[c]), NAMES)
    alone = {}
    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    alone["zns"] = zns_out(hp)
    ctx.close()
    for k, (mk, names) in make.items():
        ctx, hp = fresh()
        x = mk(ctx)(hp.rows, hp.wins, L)
        ctx.sync_check()
        alone[k] = _arrays(x, names)
        ctx.close()
    assert alone[key][3].max() > 0

    ctx, hp = fresh()
    zns(hp)
    ctx.sync_check()
    first = zns_out(hp)
    ran = [(k, make[k][0](ctx)(hp.rows, hp.wins, L)) for k in order]
    zns(hp)
    ctx.sync_check()
    assert first == alone["zns"] == zns_out(hp)
    for k, x in ran:
        for g, w_, nm in zip(_arrays(x, make[k][1]), alone[k], make[k][1]):
            assert g.tobytes() == w_.tobytes(), (k, nm)
    for k, drop in enumerate(NAMES):   # a NULL member: the others as before, the dropped array untouched
        if drop == "row":
            continue   # sl and cens need it
        part = make[key][0](ctx)
        getattr(part, drop).fill_(3)
        setattr(part.out, drop, None)
        part(hp.rows, hp.wins, L)
        ctx.sync_check()
        got = _arrays(part, NAMES)
        for j, nm in enumerate(NAMES):
            if j == k:
                assert (got[j] == 3).all(), nm
            else:
                assert got[j].tobytes() == alone[key][j].tobytes(), (drop, nm)
    ctx.close()


# ---- the PBG_BOUNDS build in a child process ----------------------------------------------------
BOUNDS_CHILD = r"""
import json, sys, numpy as np, torch
repo, spec, out = sys.argv[1:4]
sys.path.insert(0, repo); sys.path.insert(0, repo + "/tests")
from popbam_amd import _lib, workload
from tract_helpers import _params
from window_helpers import _wins_tensor
assert _lib.load().pbg_build_info() == b"bounds"
jobs, given, res = json.load(open(spec)), np.load(spec + ".npz"), {}
for i, job in enumerate(jobs):
    ctx = _lib.Context(_params(job["n"], job["masks"]), 0)
    if job["synth"]:   # (n_sites, depth, seed): called rows
        hp = workload.HotPath(ctx, workload.SynthPileup(ctx, *job["synth"]), job["wins"], _lib.PBG_S_SFS)
        hp.call()
        ctx.sync_check()
        rows = hp.rows
    else:
        rows = torch.from_numpy(given[f"rows{i}"]).cuda()
    j = getattr(workload, job["call"])(ctx, len(job["wins"]), job["max_sites"])
    j(rows, _wins_tensor(job["wins"]), job["n_rows"])
    ctx.sync_check()   # raises when the error word is not 0
    res[f"rows{i}"] = rows.cpu().numpy()
    res.update({f"{k}{i}": getattr(j, k).cpu().numpy() for k in workload.Nsl.NAMES})
    ctx.close()
np.savez(out, **res)
print("ok")
"""


def _bounds_child(tmp_path, jobs):
    """Runs the jobs through the PBG_BOUNDS build in one fresh process.  A job: call ("Nsl" / "Xpnsl"), n,
    masks, wins, n_rows, max_sites and either synth = (n_sites, depth, seed), the rows called there, or
    rows, a uint8 array of packed rows.  -> per job (its rows, its five arrays); the error word stayed 0."""
    spec, out = str(tmp_path / "bounds.json"), str(tmp_path / "bounds.npz")
    np.savez(spec + ".npz", **{f"rows{i}": j["rows"] for i, j in enumerate(jobs) if j.get("rows") is not None})
    with open(spec, "w") as f:
        json.dump([{**j, "rows": None, "synth": j.get("synth")} for j in jobs], f)
    r = subprocess.run([sys.executable, "-c", BOUNDS_CHILD, REPO, spec, out], env=dict(os.environ, POPBAM_GPU_LIB=BOUNDS_LIB),
                       capture_output=True, text=True, timeout=180)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    z = np.load(out)
    return [(z[f"rows{i}"], tuple(z[f"{k}{i}"] for k in NAMES)) for i in range(len(jobs))]
