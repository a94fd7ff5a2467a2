"""Helpers of the streamed-extension block tests (test_stream_blocks.py).

format_command (popbam_amd/csrc/stream.cpp) stages a command's extension table -- sfs --joint, sfs --dstat,
haplo --hfs, ld --rmin, haplo --nsl, haplo --xpnsl, nucdiv --snn -- a block of windows at a time, so that
its device buffer and host copy stay at kStage bytes.

source_constants / bytes_per_window / block_plan
                   the census: kStage, kRminGuess and kNslGuess read back from stream.cpp, the bytes per
                   window of each table restated, and from them a run's block size, blocks and last block
LAYOUT / counts_of / batch
                   per table the population layout, -w, region start and rows of its runs; a case is the
                   host pileup (call_edges.edge_batch over founder haplotypes), the oracle's rows for it
                   (harness.oracle_call) and its window list; the runs of a table are prefixes of one batch
checker / cells / strides
                   the table's own numpy checker (test_jsfs.ref_jsfs, ...) on the oracle's rows, over all
                   windows or sample_windows; which of its cells are neither 0 nor NA; a block's stride
ext_text           the extension columns of window w as format.cpp prints them, from the checker's arrays
                   or from a direct library call's
stream_texts / direct
                   the stream's text with and without the option (one stream, two commands, three
                   pieces) and the stream's rows; the library call over the whole window list."""
import ctypes as C
import functools
import os
import re

import numpy as np

import harness
from call_edges import edge_batch
from window_edges import founder_bits, make_params, row_bytes_for

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_CPP = os.path.join(REPO, "popbam_amd", "csrc", "stream.cpp")

# ---- the staging constants, restated from stream.cpp
K_STAGE = 64 << 20      # kStage: bytes of a table's device buffer and of its host copy
K_RMIN_GUESS = 32       # kRminGuess: intervals per (window, population) a Rmin block is sized for
K_NSL_GUESS = 256       # kNslGuess: sites per (window, chain) a tract block is sized for
WIN_LISTS = 8           # window_list: device copies of window lists a context keeps
DECAY_CAP = 1024        # pbg_common.h kDecayCap: variable sites of a decay chain kept in LDS

TABLES = ("joint", "dstat", "hfs", "rmin", "nsl", "xpnsl", "snn")
COUNTED, SEG = 2, 4
NA = "     NA"          # format.cpp Out::na
SNN_PERMS, SNN_SEED = 9, 5


def source_constants():
    """(kStage, kRminGuess, kNslGuess, window lists kept) as stream.cpp has them."""
    src = open(STREAM_CPP).read()
    a, b = re.search(r"constexpr size_t kStage = (\d+)u << (\d+);", src).groups()
    rg = re.search(r"constexpr size_t kRminGuess = (\d+);", src).group(1)
    ng = re.search(r"constexpr size_t kNslGuess = (\d+);", src).group(1)
    wl = re.search(r"if \(wl\.size\(\) >= (\d+)\)", src).group(1)
    return int(a) << int(b), int(rg), int(ng), int(wl)


def n_pairs(np_):
    return np_ * (np_ - 1) // 2


def bytes_per_window(table, pop_n):
    """What win_blocks divides kStage by (format_command's third argument of each win_blocks call)."""
    np_, n, P = len(pop_n), sum(pop_n), n_pairs(len(pop_n))
    if table == "joint":   # jC cells of 4 bytes and one double per pair
        jC = sum((pop_n[i] + 1) * (pop_n[j] + 1) for i in range(np_) for j in range(i + 1, np_))
        return jC * 4 + P * 8
    if table == "dstat":   # six int64 sums and three doubles per triple
        return P * (np_ - 2) * 72
    if table == "hfs":     # per population: hS class sizes, the class count, five doubles
        return np_ * (max(pop_n) * 4 + 44)
    if table == "rmin":
        return np_ * (4 + 8 * K_RMIN_GUESS)
    if table == "nsl":
        return np_ * (4 + 32 * K_NSL_GUESS)
    if table == "xpnsl":
        return P * (4 + 36 * K_NSL_GUESS)
    if table == "snn":     # per group a double and an int; the difference matrix of all samples
        return ((1 if np_ >= 3 else 0) + P) * 12 + n * (n - 1) // 2 * 4
    raise KeyError(table)


def block_size(table, pop_n, nw=1 << 30):
    return max(1, min(nw, K_STAGE // bytes_per_window(table, pop_n)))


def block_plan(table, pop_n, nw):
    """(block size, [(first window, windows)] of every block)."""
    size = block_size(table, pop_n, nw)
    return size, [(f, min(size, nw - f)) for f in range(0, nw, size)]


def sample_windows(runs, size):
    """The windows a costly checker runs on, one sample for all runs (window counts) of a table: every
    window within 16 of a block edge or of a run's two ends, every 16th window, and evenly spread ones up
    to 200 in all."""
    nw = max(runs)
    keep = set(range(0, nw, 16))
    for e in [0] + list(runs) + [f for r in runs for f in range(size, r, size)]:
        keep |= set(range(max(0, e - 16), min(nw, e + 16)))
    rest = [w for w in range(nw) if w not in keep]
    more = min(nw, 200) - len(keep)
    if more > 0:
        keep |= set(rest[::max(1, len(rest) // more)][:more])
    return sorted(keep)


# ---- layouts: the cheapest populations that reach a second block, with populations large enough that the
# table is not trivially 0 or NA (a population of two has no nSL pair per class and no four gametes)
class Layout:
    def __init__(self, sizes, W, pos0, founders, stretch, p, thin, sampled, k=5, balanced=0.0, drop_row=False):
        self.sizes, self.W, self.pos0, self.founders, self.stretch, self.p = sizes, W, pos0, founders, stretch, p
        self.thin = thin          # share of the rows past the first block made reference-only
        self.balanced = balanced  # populations of 4: share of (row, population) with exactly two derived samples
        self.drop_row = drop_row  # past the first block every window's second row is reference-only
        self.sampled = sampled    # the checker runs on sample_windows (test_streamed_columns_across_blocks says why)
        self.k = k


LAYOUT = {
    # 31 populations of 4: a window of 7 rows has up to 7 variable sites in each
    "nsl": Layout([4] * 31, 8, 64 * 3, 3, 24, 0.5, 0.45, False),
    # 21 populations of 2: 3,990 triples
    "dstat": Layout([2] * 21, 4, 0, 6, 16, 0.4, 0.0, True),
    # 8 populations of 4: 28 pairs of pooled chains
    "xpnsl": Layout([4] * 8, 8, 64 * 2, 3, 24, 0.5, 0.45, False),
    # 16 populations of 4: 120 pairs of 25 cells (the checker's time goes with windows x pairs, and a sample
    # of 200 windows costs least with few pairs)
    "joint": Layout([4] * 16, 4, 0, 8, 16, 0.4, 0.0, True),
    # 3 populations of 42: the matrix of 126 samples is the table's bulk
    "snn": Layout([42] * 3, 4, 64 * 5, 4, 12, 0.4, 0.0, True),
    # one population of 63 and 63 of one
    "hfs": Layout([63] + [1] * 63, 4, 0, 4, 12, 0.4, 0.0, False),
    # 31 populations of 4 (four gametes need four samples; at most 31 such populations fit 126 samples, hence
    # the 8,326 windows of a block): windows of 3 rows and up to 2 intervals in the first block, of 2 variable
    # rows and one interval past it; half of the columns split a population two and two, which is what makes
    # two sites incompatible often enough
    "rmin": Layout([4] * 31, 4, 64 * 7, 64, 4, 0.5, 0.0, False, balanced=0.5, drop_row=True),
}
EVERY_COUNT = ("nsl", "dstat", "xpnsl")   # size, size + 1, 2 size, 2 size + 3; the others size + k


def counts_of(table):
    """{run name: windows} of the table's runs."""
    lay = LAYOUT[table]
    size = block_size(table, lay.sizes)
    if table in EVERY_COUNT:
        return {"size": size, "size+1": size + 1, "2size": 2 * size, "2size+3": 2 * size + 3}
    return {f"size+{lay.k}": size + lay.k}


CASES = [(t, r) for t in TABLES for r in counts_of(t)]
CASE_IDS = [f"{t}-{r}" for t, r in CASES]


class Batch:
    """A table's host pileup over the rows of its longest run, the oracle's rows, and the windows."""

    def __init__(self, table):
        from popbam_amd import workload
        lay = self.lay = LAYOUT[table]
        self.table = table
        self.n, self.sizes = sum(lay.sizes), list(lay.sizes)
        self.size = block_size(table, lay.sizes)
        self.nw_max = max(counts_of(table).values())
        # main_<cmd>'s windows drop their last base and the trailing partial window: nw = (L - 1) / W
        self.L = (self.nw_max * lay.W + 1 + 63) // 64 * 64
        rng = np.random.default_rng([0x57B10C5] + [ord(c) for c in table])
        bits = founder_bits(rng, self.L, self.n, lay.founders, lay.stretch, lay.p)
        if lay.balanced:
            assert set(lay.sizes) == {4}
            splits = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [0, 1, 1, 0], [1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 1]], np.uint8)
            use = rng.random((self.L, len(lay.sizes))) < lay.balanced
            bits.reshape(self.L, -1, 4)[use] = splits[rng.integers(0, 6, int(use.sum()))]
        past = np.arange(self.L) >= self.size * lay.W
        sparse = past & (rng.random(self.L) < lay.thin)
        if lay.drop_row:
            sparse |= past & (np.arange(self.L) % lay.W == 1)
        bits[sparse] = 0
        # an all-alternative sample needs 9 reads (with these base qualities the caller calls none of 8 or
        # fewer), an all-reference one min_depth = 3
        depth = np.where(bits > 0, rng.integers(9, 11, (self.L, self.n)), rng.integers(3, 5, (self.L, self.n)))
        self.batch = edge_batch(rng.integers(0, 4, self.L), np.zeros(self.L, np.int64), depth, bits, rng)
        self.params = make_params(self.n, self.sizes)
        self.masks = [self.params.get_pop_mask(i) for i in range(len(self.sizes))]
        self.kb = harness.key_batch(self.batch, self.params)
        _, self.types, _, self.flags = harness.oracle_call(harness.oracle_params_from(self.params), self.batch)
        self.rows = harness.rows_from_oracle(self.types, self.flags, row_bytes_for(self.n))
        self.wins = workload.reference_windows(0, self.nw_max * lay.W + 1, lay.W)   # as rows
        self.pops = [f"p{i}" for i in range(len(self.sizes))]
        seg = np.concatenate([[0], np.cumsum((self.flags & SEG) > 0)])
        self.seg_rows = [int(seg[b] - seg[a]) for a, b in self.wins]
        self._checked = {}

    def end_for(self, nw):
        """The command's region end (contig position) that gives nw windows."""
        return self.lay.pos0 + nw * self.lay.W + 1

    # ---- the checker on the oracle's rows
    def checker(self, idx):
        """The table's checker over the windows `idx` -> its arrays, first axis len(idx)."""
        key = tuple(idx)
        if key not in self._checked:
            self._checked[key] = _checker(self, [self.wins[w] for w in idx])
        return self._checked[key]

    def checker_for(self, nw):
        """(windows, arrays) of a run of nw windows: the rows of the table's one checker run (over all
        windows of its longest run, or over sample_windows) that the run has."""
        every = sample_windows(list(counts_of(self.table).values()), self.size) if self.lay.sampled else list(range(self.nw_max))
        full = self.checker(every)
        k = sum(w < nw for w in every)   # ascending
        return every[:k], tuple(a[:k] for a in full)


@functools.lru_cache(maxsize=None)
def batch(table):
    return Batch(table)


def _checker(b, wins):
    pop_n, t = b.sizes, b.table
    if t == "joint":
        from test_jsfs import ref_jsfs
        return ref_jsfs(b.types, b.flags, b.masks, pop_n, wins)
    if t == "dstat":
        from test_dstat import all_triples, ref_dstat
        return ref_dstat(b.types, b.flags, b.masks, pop_n, wins, all_triples(len(pop_n)))
    if t == "hfs":
        from test_hfs import ref_hfs
        return ref_hfs(b.types, b.flags, b.masks, pop_n, b.n, wins)
    if t == "rmin":
        from test_rmin import ref_rmin
        return ref_rmin(b.types, b.flags, b.masks, pop_n, wins, 1, b.lay.W - 2)   # at most rows - 1 intervals
    if t == "nsl":
        from test_nsl import ref_nsl
        return ref_nsl(b.types, b.flags, b.masks, pop_n, wins, b.lay.W - 1)
    if t == "xpnsl":
        from test_xpnsl import ref_xpnsl
        return ref_xpnsl(b.types, b.flags, b.masks, pop_n, wins, b.lay.W - 1)
    if t == "snn":
        from test_snn import default_groups, ref_snn
        return ref_snn(b.types, b.flags, b.n, b.masks, wins, default_groups(len(pop_n)), SNN_PERMS, SNN_SEED, b.lay.pos0)
    raise KeyError(t)


def cells(table, arrays):
    """[windows, cells] bool: the checker's printed cells that are neither 0 nor NA."""
    if table == "joint":
        return ~np.isnan(arrays[2]) & (arrays[2] != 0)                 # Fst per pair
    if table == "dstat":
        return ~np.isnan(arrays[1]) & (arrays[1] != 0)                 # D per triple
    if table == "hfs":
        h = arrays[4].reshape(len(arrays[4]), -1)                      # H1, H12, H123, H2H1, Hd per population
        return ~np.isnan(h) & (h != 0)
    if table == "rmin":
        return arrays[0] > 0                                           # Rmin per population (0: rint is NA)
    if table in ("nsl", "xpnsl"):
        return arrays[0] > 0                                           # sites per chain (0: the column is NA)
    if table == "snn":
        return arrays[1] != 0                                          # Snn per group
    raise KeyError(table)


def counts(table, arrays):
    """[windows, chains] of the number whose largest value in a block is that block's stride."""
    return arrays[0]   # rmin of ref_rmin; n_var of ref_nsl and ref_xpnsl


# ---- the extension columns as format.cpp prints them
def _f(v):
    return NA if v != v else "%.5f" % v


@functools.lru_cache(maxsize=None)
def _dstat_labels(pops):
    from test_dstat import all_triples
    labs = [f"[{pops[i]},{pops[j]},{pops[l]}]:\t" for i, j, l in all_triples(len(pops))]
    return [("\tD" + x, "\tfd" + x, "\tfdM" + x, "\tdsum" + x) for x in labs]


def ext_text(b, arrays, k, w):
    """The columns the option appends to window w's line, from row k of `arrays` (the checker's layout;
    a direct library call's arrays have it too)."""
    t, pops, pop_n, pos0 = b.table, b.pops, b.sizes, b.lay.pos0
    np_ = len(pops)
    out = []
    if t == "joint":
        from test_jsfs import pair_list, pair_offsets
        cells_, fst = arrays[0][k].tolist(), arrays[2][k].tolist()
        off = pair_offsets(pop_n)
        for p, (i, j) in enumerate(pair_list(np_)):
            out.append(f"\tfst[{pops[i]},{pops[j]}]:\t{_f(fst[p])}\tjsfs[{pops[i]},{pops[j]}]:\t"
                       + ",".join(map(str, cells_[off[p]:off[p + 1]])))
    elif t == "dstat":
        sums = arrays[0][k].tolist()
        d, fd, fdm = ([NA if v != v else "%.5f" % v for v in a[k].tolist()] for a in arrays[1:])
        out = [a + x + c + y + e + z + g + ",".join(map(str, s)) for (a, c, e, g), x, y, z, s in zip(_dstat_labels(tuple(pops)), d, fd, fdm, sums)]
    elif t == "hfs":
        from test_hfs import HNAMES
        kk, cnt, h = arrays[0][k].tolist(), arrays[1][k].tolist(), arrays[4][k].tolist()
        for i, p in enumerate(pops):
            out.append("".join(f"\t{nm}[{p}]:\t{_f(v)}" for nm, v in zip(HNAMES, h[i]))
                       + f"\thfs[{p}]:\t" + ",".join(map(str, cnt[i][:kk[i]])))
    elif t == "rmin":
        rmin, cuts = arrays[0][k].tolist(), arrays[2][k].tolist()
        for i, p in enumerate(pops):
            ivs = ",".join(f"{a + pos0 + 1}-{c + pos0 + 1}" for a, c in cuts[i][:rmin[i]]) if rmin[i] > 0 else "NA"
            out.append(f"\tRmin[{p}]:\t{rmin[i]}\trint[{p}]:\t{ivs}")
    elif t == "nsl":
        from test_nsl import value_text
        n_var, row, m, sl, cens = (a[k].tolist() for a in arrays)
        for i, p in enumerate(pops):
            toks = [f"{row[i][s] + pos0 + 1}:{m[i][s]}:{value_text(pop_n[i], m[i][s], *sl[i][s])}:{sum(cens[i][s])}"
                    for s in range(n_var[i])]
            out.append(f"\tnsl[{p}]:\t" + (",".join(toks) if toks else "NA"))
    elif t == "xpnsl":
        from test_xpnsl import pairs_of, value_text
        n_var, row, m, sl, cens = (a[k].tolist() for a in arrays)
        for x, (i, j) in enumerate(pairs_of(np_)):
            toks = [f"{row[x][s] + pos0 + 1}:{m[x][s][0]}:{m[x][s][1]}:{value_text(pop_n[i], pop_n[j], *sl[x][s])}:{sum(cens[x][s])}"
                    for s in range(n_var[x])]
            out.append(f"\txpnsl[{pops[i]},{pops[j]}]:\t" + (",".join(toks) if toks else "NA"))
    elif t == "snn":
        from test_snn import _group_names
        snn, ge = arrays[1][k].tolist(), arrays[3][k].tolist()
        seg = b.seg_rows[w] > 0
        for e, nm in enumerate(_group_names(pops)):
            v = "%.5f" % snn[e] if seg else NA
            p = "%.5f" % (float(ge[e] + 1) / float(SNN_PERMS + 1)) if seg else NA
            out.append(f"\tsnn[{nm}]:\t{v}\tpsnn[{nm}]:\t{p}")
    return "".join(out)


# ---- the device
CMD = {   # table -> (pbg_cmd.cmd, the option's bits of pbg_cmd.output, pbg_cmd.hfs)
    "joint": (6, 2, 0), "dstat": (6, 4, 0), "hfs": (1, 0, 1), "rmin": (5, 4, 0), "nsl": (1, 4, 0), "xpnsl": (1, 8, 0),
    "snn": (4, 1 | SNN_PERMS << 1 | SNN_SEED << 17, 0),
}


def command(keep, cmd, output, beg, end, win_size, hfs=0, decay=(0, 0), min_sites=10):
    """A pbg_cmd over [beg, end) with -w win_size (0: no windows); `keep` holds the name arrays."""
    from popbam_amd import _lib
    c = _lib.PbgCmd()
    c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq, c.hfs = cmd, output, min_sites, 10, 1, hfs
    c.windowed, c.win_size, c.beg, c.end = (1, win_size, beg, end) if win_size else (0, 0, beg, end)
    c.decay_bin, c.decay_bins = decay
    c.chr_name = keep[0]
    c.sample_names = C.cast(keep[1], C.POINTER(C.c_char_p))
    c.pop_names = C.cast(keep[2], C.POINTER(C.c_char_p))
    c.refid = b"ref"
    return c


def names(n, pops):
    return [b"chr1", (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)]), (C.c_char_p * len(pops))(*[p.encode() for p in pops])]


def run_stream(ctx, kb, L, n, pos0, cmds, pieces=3):
    """The host key batch pushed in `pieces` pieces of whole 64-position blocks -> (the stream's rows on the
    host, the text of every command)."""
    from popbam_amd import _lib
    rb = ctx.row_bytes
    k2, rq2, boff = kb["k"].reshape(L, n), kb["rmsq"].reshape(L, n), kb["block_off"]
    nblk = (L + 63) // 64
    piece = 64 * max(1, (nblk + pieces - 1) // pieces)
    rows = np.zeros(L * rb, np.uint8)
    held = []
    with _lib.Stream(ctx, cmds, pos0, L) as st:
        for a in range(0, L, piece):
            e = min(L, a + piece)
            k0, k1 = int(boff[a // 64]), int(boff[(e + 63) // 64])
            arr = (np.ascontiguousarray(kb["ref"][a:e]), np.ascontiguousarray(k2[a:e]), np.ascontiguousarray(rq2[a:e]),
                   np.ascontiguousarray(kb["keys"][k0:k1]) if k1 > k0 else np.zeros(8, np.uint16))
            held.append(arr)   # pushed asynchronously: alive until finish
            st.push(_lib.PbgPileup(e - a, pos0 + a, arr[0].ctypes.data, arr[1].ctypes.data, arr[2].ctypes.data, None,
                                   arr[3].ctypes.data))
        assert len(held) >= min(pieces, nblk)
        st.finish()
        st.rows_into(rows.ctypes.data, rows.size)
        texts = [st.text(i) for i in range(len(cmds))]
    return rows, texts


def stream_texts(ctx, b, nw):
    """One stream over the batch with the table's command without and with its option, nw windows each."""
    cmd, bits, hfs = CMD[b.table]
    keep = names(b.n, b.pops)
    cmds = [command(keep, cmd, 0, b.lay.pos0, b.end_for(nw), b.lay.W),
            command(keep, cmd, bits, b.lay.pos0, b.end_for(nw), b.lay.W, hfs)]
    rows, (plain, ours) = run_stream(ctx, b.kb, b.L, b.n, b.lay.pos0, cmds)
    return rows, plain, ours


def direct(ctx, b, nw):
    """The table's entry point once over the whole list of nw windows (no blocks) on the oracle's rows ->
    arrays in the checker's layout (members the text does not print are None)."""
    import torch
    from popbam_amd import workload
    from window_helpers import _arrays, _wins_tensor
    rows = torch.from_numpy(b.rows.copy()).cuda()
    wt = _wins_tensor(b.wins[:nw])
    t = b.table
    if t == "joint":
        j = workload.JointSfs(ctx, nw)(rows, wt, b.L)
        names_ = ("cells", "diffs", "fst")
    elif t == "dstat":
        from test_dstat import all_triples
        j = workload.DStat(ctx, nw, all_triples(len(b.sizes)))(rows, wt, b.L)
        names_ = ("sums", "d", "fd", "fdm")
    elif t == "rmin":
        j = workload.Rmin(ctx, nw, 1, b.lay.W - 2)(rows, wt, b.L)
        names_ = ("rmin", "n_var", "cuts")
    elif t == "snn":
        j = workload.Snn(ctx, nw, workload.Snn.default_groups(len(b.sizes)), SNN_PERMS, SNN_SEED, b.lay.pos0)(rows, wt, b.L)
        names_ = ("diff", "snn", "near", "ge")
    else:
        raise KeyError(t)
    ctx.sync_check()
    return _arrays(j, names_)
