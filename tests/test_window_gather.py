"""pbg_window_stats on crafted rows whose count is no multiple of the rows per 16-byte word: the
ordered gather's partial last word (pbg_rows.h: gather_rows_in_order, load_row_word), the window
edges inside a word, and its second pass into the pool, against the oracle's text."""
import ctypes as C
import types as pytypes

import numpy as np
import pytest

import harness
from test_gpu_scale import _ctx, _oracle_text, _window_text
from window_helpers import PARTIAL_WORD_CASES, _random_types, _wins_tensor, partial_rows

pytestmark = pytest.mark.gpu

COUNTED, SEG = 2, 4
STATS = [(0x001, 4, 0), (0x002, 6, 0), (0x004, 5, 0)]   # (PBG_S_NUCDIV / SFS / ZNS, popbam_func_t, -o)


@pytest.mark.parametrize("n,words", PARTIAL_WORD_CASES)
def test_window_stats_partial_last_word(gpu_lib, n, words):
    """n_rows = L ends inside a 16-byte word.  The device buffer goes on to the end of that word and
    one word further, and every row from L on is counted and segregating with every sample set: a
    read past n_rows changes num_sites and segsites instead of passing silently.  The short input
    has random flags; in the 513-word input every row segregates, so that each trip of the gather
    is full and, at 12 samples, one window holds 4,107 segregating rows: above every LDS capacity,
    which sends the list through the gather's second pass into the pool."""
    import torch
    from popbam_amd import _lib, workload
    L, more = partial_rows(n, words)
    ctx, params = _ctx(n, 2)
    R = 16 // ctx.row_bytes
    assert R == 1 or L % R != 0   # (a 16-byte row is a word of its own: the padding alone tells there)
    Lpad = ((L + R - 1) // R + 1) * R
    rng = np.random.default_rng(1000 + n)
    types = _random_types(rng, Lpad, n)
    if words is None:
        counted = rng.random(Lpad) < 0.9
        flags = np.where(counted, np.where(rng.random(Lpad) < 0.5, COUNTED | SEG, COUNTED), 0).astype(np.uint8)
    else:
        flags = np.full(Lpad, COUNTED | SEG, np.uint8)
    flags[L:] = COUNTED | SEG
    if n > 64:
        types[L:, 0], types[L:, 1] = np.uint64((1 << 64) - 1), np.uint64((1 << (n - 64)) - 1)
    else:
        types[L:] = np.uint64((1 << n) - 1)
    rows = torch.from_numpy(harness.rows_from_oracle(types, flags, ctx.row_bytes).copy()).cuda()
    assert rows.numel() == Lpad * ctx.row_bytes and rows.data_ptr() % 16 == 0
    wins = [(0, L), (0, 1), (L - 1, L), (5, 5), (3, L - 2), (R + 1, 2 * R + 1)] + more
    out = workload.WindowOutputs(len(wins), n, 2, "cuda", ctx.sfs_stride)
    o = out.struct(list(out.t))
    so = _lib.PbgStatOpts(sum(s for s, _, _ in STATS), 1, 0, 0)
    wt = _wins_tensor(wins)
    ctx.check(ctx.lib.pbg_window_stats(ctx.h, rows.data_ptr(), L, wt.data_ptr(), len(wins), C.byref(so), C.byref(o),
                                       workload.stream_handle()), "pbg_window_stats")
    ctx.sync_check()
    torch.cuda.synchronize()
    hp = pytypes.SimpleNamespace(out=out)
    for _, cmd_id, output in STATS:
        gpu = _window_text(ctx, params, hp, cmd_id, output, wins)
        orc = _oracle_text(params, types[:L], flags[:L], cmd_id, output, wins)
        assert gpu == orc, (n, words, cmd_id)
    seg = out.t["segsites"].cpu().numpy()
    assert seg[0] == int(((flags[:L] & SEG) > 0).sum()) and seg[3] == 0
    if words is not None and n == 12:
        assert L == 4107 and seg[0] == L and seg[0] > 256   # past every segcap: the pool pass ran
    ctx.close()
