"""The edges of the tract walk that pbg_window_nsl and pbg_window_xpnsl share (pbg_tract.h), which no
other input reaches on purpose.  Both calls, bitwise against test_nsl.py's and test_xpnsl.py's checkers.

Site-batch edges: chains of exactly V = 1, 63, 64, 65, 127, 128 and 129 sites -- the forward walk's
batches of 64 sites and the backward walk's first trip at ((V - 1) / 64) * 64.  Every crafted row is
segregating and variable in every population (so in every pooled pair too), hence a window of V rows is
a chain of V sites in every chain of both calls; the windows start at row 0 and at row 5, inside a
16-byte word of 2-, 4- and 8-byte rows.

Pair-table edges, the lane stride of 64 in the pair loop and in the table fill: nSL on populations of 11
and 12 samples (55 and 66 pairs), XP-nSL on sides of 8 + 9 (exactly 64 pairs) and 11 + 5 (65).

Samples copy founders over stretches of 150 rows, so tracts are longer than a batch."""
import os

import numpy as np
import pytest

from test_nsl import ref_nsl
from test_xpnsl import ref_xpnsl
from tract_helpers import BOUNDS_LIB, COUNTED, SEG, _assert_same, _bounds_child, _crafted, _run_nsl, _run_xpnsl
from window_helpers import _blocks

BATCH_V = (1, 63, 64, 65, 127, 128, 129)
L, STRETCH = 400, 150
CASES = {   # name -> population sizes
    "n12": [6, 6],      # 2-byte rows
    "n16": [11, 5],     # XP-nSL: 55 + 10 = 65 pairs
    "n17": [8, 9],      # XP-nSL: 28 + 36 = 64 pairs
    "n23": [11, 12],    # nSL: 55 and 66 pairs
    "n66": [40, 26],    # 16-byte rows, population 0 within the first word, population 1 across both
}
WINS = [(s, s + v) for v in BATCH_V for s in (0, 5)] + [(0, L), (3, L - 1)]
_cases = {}


def _rows(sizes, seed):
    """Every sample copies one of four founders, the copy changing every STRETCH rows; in every population
    sample 0 copies founder 0 and sample 1 founder 1, whose bits differ at every row."""
    rng = np.random.default_rng(seed)
    n = sum(sizes)
    first = np.cumsum([0] + sizes[:-1])
    ints = []
    for r0 in range(0, L, STRETCH):
        src = rng.integers(0, 4, n)
        src[first], src[first + 1] = 0, 1
        for _ in range(min(STRETCH, L - r0)):
            fb = rng.integers(0, 2, 4)
            fb[1] = 1 - fb[0]
            ints.append(sum(int(fb[src[s]]) << s for s in range(n)))
    types = np.array([[x & ((1 << 64) - 1), x >> 64] for x in ints], np.uint64)
    return types if n > 64 else types[:, 0].copy()


def _case(name):
    """(samples, masks, types, flags, the nSL checker's arrays, the XP-nSL checker's), computed once."""
    if name not in _cases:
        sizes = CASES[name]
        n, masks = sum(sizes), _blocks(sizes)
        types, flags = _rows(sizes, 900 + n), np.full(L, COUNTED | SEG, np.uint8)
        _cases[name] = (n, masks, types, flags, ref_nsl(types, flags, masks, sizes, WINS, L),
                        ref_xpnsl(types, flags, masks, sizes, WINS, L))
    return _cases[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_batch_edge_is_met_in_every_chain(name):
    n, masks, types, flags, want_nsl, want_xp = _case(name)
    for want in (want_nsl, want_xp):
        n_var = want[0]
        assert n_var.shape[1] >= 1
        for w, (a, b) in enumerate(WINS):
            assert (n_var[w] == b - a).all(), (name, a, b)   # every row is a site of every chain
        assert {int(v) for v in n_var[:2 * len(BATCH_V)].ravel()} == set(BATCH_V)
        assert want[3][-2].max() > 64   # tracts longer than a batch
    pairs = {nm: [s * (s - 1) // 2 for s in sz] for nm, sz in CASES.items()}
    assert pairs["n23"] == [55, 66] and sum(pairs["n17"]) == 64 and sum(pairs["n16"]) == 65


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_tract_edges_match_the_checkers(gpu_lib, name):
    n, masks, types, flags, want_nsl, want_xp = _case(name)
    ctx, params, rows = _crafted(n, masks, types, flags)
    _assert_same(_run_nsl(ctx, rows, L, WINS, L), want_nsl, ("nsl", name))
    _assert_same(_run_xpnsl(ctx, rows, L, WINS, L), want_xp, ("xpnsl", name))
    # max_sites = 129: the longest of the batch-edge chains fills its slots to the last one
    edge = WINS[:2 * len(BATCH_V)]
    for run, want in ((_run_nsl, want_nsl), (_run_xpnsl, want_xp)):
        got = run(ctx, rows, L, edge, max(BATCH_V))
        _assert_same(got, tuple(x[:len(edge), :, :max(BATCH_V)] if x.ndim > 2 else x[:len(edge)] for x in want), (name, "129"))
    ctx.close()


@pytest.mark.gpu
def test_tract_edges_under_the_bounds_build(gpu_lib, tmp_path):
    """The same cases once through the PBG_BOUNDS build (one fresh process): the checkers' numbers, and the
    error word stays 0."""
    assert os.path.exists(BOUNDS_LIB), "the bounds build is not there: the Makefile's `bounds` target builds it"
    jobs, wants = [], []
    for name in CASES:
        n, masks, types, flags, want_nsl, want_xp = _case(name)
        ctx, params, dev = _crafted(n, masks, types, flags)
        rows = dev.cpu().numpy()
        ctx.close()
        for call, want in (("Nsl", want_nsl), ("Xpnsl", want_xp)):
            jobs.append(dict(call=call, n=n, masks=masks, wins=WINS, n_rows=L, max_sites=L, rows=rows))
            wants.append((name, call, want))
    for (brows, got), (name, call, want), job in zip(_bounds_child(tmp_path, jobs), wants, jobs):
        assert np.array_equal(brows, job["rows"])
        _assert_same(got, want, ("bounds", name, call))
