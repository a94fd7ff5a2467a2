"""Helpers shared by the tests of the per-window side tables (test_ld_decay.py, test_jsfs.py,
test_dstat.py, test_hfs.py): bit arithmetic for the checkers, crafted inputs, and the native
command line.  The checkers themselves (`ref_*`) stay with their tests.  Also the two text
printers of the pbg_window_stats tests (test_gpu_scale.py, test_window_gather.py, test_window_edges.py,
test_hfs.py): window_text (pbg_format over the device outputs) and oracle_text (the oracle's windows
over given sites)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fixtures
import harness

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "bin", "popbam")


def popcount(x):
    """Per-element popcount of a uint64 array."""
    b = np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8).reshape(-1, 8)
    return np.unpackbits(b, axis=1).sum(axis=1).astype(np.int64)


def mask_words(types):
    """types ([L] u64, or [L, 2] for n > 64) -> (lo, hi) u64 arrays."""
    types = np.asarray(types, dtype=np.uint64)
    if types.ndim == 2:
        return types[:, 0].copy(), types[:, 1].copy()
    return types, np.zeros(len(types), np.uint64)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _random_types(rng, L, n):
    if n <= 64:
        return rng.integers(0, 1 << n, L, dtype=np.uint64)
    t = np.zeros((L, 2), np.uint64)
    t[:, 0] = rng.integers(0, 1 << 64, L, dtype=np.uint64)
    t[:, 1] = rng.integers(0, 1 << (n - 64), L, dtype=np.uint64)
    return t


def _blocks(sizes):
    """Contiguous population masks of the given sizes."""
    masks, at = [], 0
    for s in sizes:
        masks.append(((1 << s) - 1) << at)
        at += s
    return masks


def _pop_masks(params):
    return ([params.get_pop_mask(i) for i in range(params.n_pops)], [params.pop_n[i] for i in range(params.n_pops)])


def _wins_tensor(wins):
    import torch
    return torch.tensor([x for ab in wins for x in ab], dtype=torch.int32).reshape(-1, 2).cuda()


def _arrays(x, names):
    return tuple(getattr(x, k).cpu().numpy().copy() for k in names)


def _native(argv, timeout=120):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    r = subprocess.run([BIN, *argv], capture_output=True, timeout=timeout, env=e)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def _argv(name, cs):
    d = fixtures.load_case(name)["dir"]
    a = cs["args"]
    return [a[0], "-f", os.path.join(d, "ref.fa")] + list(a[1:]) + [os.path.join(d, "in.bam"), cs["region"]]


# The *_partial_last_word tests: (n, words).  words None is the short input of 64 * 5 + 3 rows.  With
# 513 16-byte words of rows plus three rows, every row segregating, the first wave of the row stream
# (pbg_rows.h) goes round its loop three times (words 0.., 256.., 512..) with a full queue in the first
# two, and a load-ahead of two words reaches past the window's end; n = 12, 24, 48, 96 are 2-, 4-, 8-
# and 16-byte rows.
PARTIAL_WORD_CASES = ([pytest.param(n, None, id=str(n)) for n in (12, 24, 48, 96)]
                      + [pytest.param(n, 513, id=f"{n}-513words") for n in (12, 24, 48, 96)])


def partial_rows(n, words):
    """(L, extra windows) of a *_partial_last_word case: L is no multiple of the R rows per word; the
    long input adds a window of two rows, the last row of word 255 (the last wave's full queue) and the
    first of word 256 (the first wave's second trip)."""
    if words is None:
        return 64 * 5 + 3, []
    R = 16 // (2 if n <= 14 else 4 if n <= 30 else 8 if n <= 62 else 16)
    return words * R + 3, [(256 * R - 1, 256 * R + 1)]


def _names(c, n, np_):
    """chr1 / s<i> / p<i> / ref into a command struct; the arrays returned must outlive the call."""
    c.chr_name = b"chr1"
    sn = (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)])
    pn = (C.c_char_p * np_)(*[f"p{i}".encode() for i in range(np_)])
    c.sample_names = C.cast(sn, C.POINTER(C.c_char_p))
    c.pop_names = C.cast(pn, C.POINTER(C.c_char_p))
    c.refid = b"ref"
    return sn, pn


def window_text(ctx, params, hp, cmd_id, output, windows, min_freq=1, jc=0, min_snps=10, outidx=0,
                min_sites=10):
    """Format the GPU window outputs (`hp.out.t`, a workload.WindowOutputs' tensors) with the
    library's print_<stat> (pbg_format)."""
    from popbam_amd import _lib
    host = {k: v.cpu().numpy() for k, v in hp.out.t.items()}
    o = _lib.PbgWindowOut()
    for k in [f for f, _ in _lib.PbgWindowOut._fields_]:
        setattr(o, k, host[k].ctypes.data)
    c = _lib.PbgCmd()
    c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq, c.jc = cmd_id, output, min_sites, min_snps, min_freq, jc
    c.outidx = outidx
    keep = _names(c, params.n_samples, params.n_pops)
    wb = np.array([a for a, _ in windows], np.int32)
    we = np.array([b for _, b in windows], np.int32)
    cap = 1 << 24
    buf = C.create_string_buffer(cap)
    need = C.c_size_t()
    r = ctx.lib.pbg_format(ctx.h, C.byref(c), C.byref(o), len(windows), wb.ctypes.data, we.ctypes.data, buf, cap,
                           C.byref(need))
    ctx.check(r, "pbg_format")
    del keep
    return buf.value.decode()


def oracle_text(params, types, flags, cmd_id, output, windows, min_freq=1, jc=0, min_snps=10, outidx=0, min_sites=10):
    """The oracle's text of one command over the windows of given sites (orc_windows_from_sites)."""
    p = harness.oracle_params_from(params)
    c = harness.OrcCmd()
    c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq, c.jc = cmd_id, output, min_sites, min_snps, min_freq, jc
    c.outidx = outidx
    keep = _names(c, params.n_samples, params.n_pops)
    wb = np.array([a for a, _ in windows], np.int32)
    we = np.array([b for _, b in windows], np.int32)
    types, flags = np.ascontiguousarray(types), np.ascontiguousarray(flags)
    cap = 1 << 24
    buf = C.create_string_buffer(cap)
    r = harness.oracle().orc_windows_from_sites(C.byref(p), C.byref(c), types.ctypes.data, flags.ctypes.data,
                                                len(windows), wb.ctypes.data, we.ctypes.data, buf, cap)
    assert r >= 0
    del keep
    return buf.value.decode()
