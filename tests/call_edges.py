"""Helpers of the call-pipeline edge tests (test_call_edges.py, test_gpu_mixed_quality.py).

edge_batch         a raw batch of per-task depth and read pattern (`kind`), built in numpy
check_call_routes  one batch through the call pipeline's routes, each bitwise against the CPU
                   oracle (orc_call_sites): a) rows only, b) consensus words, c) the stream,
                   d) the stream with compact pieces
census             what a packed key batch asks of the scan's fixed capacities, computed on the
                   CPU from the limits restated below
case               the named batches of test_call_edges.py with their oracle results, built once
                   per process (the bounds-build child process rebuilds them by name)."""
import ctypes as C
import functools

import numpy as np

import harness

# ---- the call pipeline's limits, restated from the source
SITE_BLOCK = 64          # include/popbam_gpu.h PBG_SITE_BLOCK: one scan wave per 64-position block
ROUND_TASKS = 128        # call_kernel.hip:888-889: rounds of 128 (position, sample) tasks
ROUND_KEYS = 512 * 8     # call_kernel.hip:910 kScanChunks: 512 16-byte chunks = 4096 keys a round may stage
LIST = 256               # call_kernel.hip:912 kScanList: list entries per wave
LIST_NARROW = 192        # call_kernel.hip:913 kScanListNarrow ...
NARROW_N = 12            # call_kernel.hip:914 kNarrowN: ... at most this many samples
LIST_WIDE = 448          # call_kernel.hip:915 kScanListWide: above LDS_INFO_N samples
LDS_INFO_N = 24          # call_kernel.hip:923 kLdsInfoN: up to here the info bytes live in LDS
FAST_MAX = 32            # call_kernel.hip:927 kFastMax (pbg_common.h PBG_FAST_MAX): reference-only up to 32 keys
NET_MAX = 16             # call_kernel.hip:901-904: at most 16 keys: one_error_ref / queue record / 16-wire network
LIST_OFF_MAX = 1 << 21   # call_kernel.hip:932 kListOffMax: a list entry's 21-bit first-key offset


def blk_cap(n):
    """Queue records of one block's region (api.cpp:456)."""
    return SITE_BLOCK * n * 3 // 16 + 32


def list_cap(n):
    """The wave's list entries (call_kernel.hip:912-915)."""
    return LIST_NARROW if n <= NARROW_N else LIST if n <= LDS_INFO_N else LIST_WIDE


def task_cap(L, n):
    """Entries of the deep list a fresh context allocates for a batch of L positions (api.cpp:457)."""
    nblk = (L + SITE_BLOCK - 1) // SITE_BLOCK
    return max(nblk * blk_cap(n), min(L * n // 32 + 65536, 0xFFFFFFFF))


# ---- batches
REF_UPPER = np.frombuffer(b"ACGT", np.uint8)
REF_LOWER = np.frombuffer(b"acgt", np.uint8)


def edge_batch(ref_idx, lower, depth, kind, rng, max_depth=None, illumina=False):
    """The raw batch dict harness.oracle_call / harness.key_batch take ('ref', 'depth' u16, 'reads'
    u32; a read word is baseQ | mapQ << 8 | nt16 << 16 | strand << 20, include/popbam_feed.h).

    ref_idx[L]  reference base 0..3 (A/C/G/T); lower[L]: 0 upper-case, 1 lower-case, 2 'N'
    depth[L,n]  reads per task (capped at max_depth when given: the pileup's partition keeps a
                sample's first max_depth reads); kind[L,n] their pattern:
      0 all reference                      3 each read alternative with p = 0.5
      1 all alternative                    4 each read a random base with p = 0.1
      2 one alternative read               5 all alternative but one reference read
    One alternative base per position (uniform over the three others), shared by its samples.  The
    single read of kinds 2 and 5 sits at index 0, at index 1 or anywhere, a third each (the list
    pass takes key 0's base for the majority unless key 0 alone differs).  baseQ uniform in 13..41
    and mapQ 60 or (p = 0.1) 20 pass the default filters, so k == depth; strands are random.
    illumina: the stored baseQ carries the Illumina 1.3+ offset of 31 that flag 0x02 takes off
    again (pbg_key.h), so k == depth under that flag too.  The dict also keeps `kind` ([L,n])."""
    ref_idx = np.asarray(ref_idx, np.int64)
    lower = np.asarray(lower, np.int64)
    dep = np.asarray(depth, np.int64)
    if max_depth is not None:
        dep = np.minimum(dep, max_depth)
    L, n = dep.shape
    T = L * n
    d = dep.reshape(T)
    knd = np.asarray(kind, np.int64).reshape(T)
    alt = (ref_idx + rng.integers(1, 4, L)) & 3
    R = int(d.sum())
    start = np.cumsum(d) - d
    task = np.repeat(np.arange(T), d)
    within = np.arange(R) - start[task]
    u = rng.integers(0, 3, T)
    pick = np.where(u == 0, 0, np.where(u == 1, np.minimum(1, d - 1), rng.integers(0, np.maximum(d, 1))))
    rk, at_pick = knd[task], within == pick[task]
    is_alt = (rk == 1) | ((rk == 2) & at_pick) | ((rk == 3) & (rng.random(R) < 0.5)) | ((rk == 5) & ~at_pick)
    pos = task // n
    base = np.where(is_alt, alt[pos], ref_idx[pos])
    base = np.where((rk == 4) & (rng.random(R) < 0.1), rng.integers(0, 4, R), base)
    bq = rng.integers(13, 42, R) + (31 if illumina else 0)
    mq = np.where(rng.random(R) < 0.1, 20, 60)
    reads = bq | (mq << 8) | ((1 << base) << 16) | (rng.integers(0, 2, R) << 20)
    ref = np.where(lower == 2, ord("N"), np.where(lower == 1, REF_LOWER[ref_idx], REF_UPPER[ref_idx]))
    return {"ref": ref.astype(np.uint8), "depth": np.ascontiguousarray(dep, dtype=np.uint16),
            "reads": reads.astype(np.uint32), "kind": knd.reshape(L, n)}


# ---- census
def census(key_batch, n):
    """What the packed key batch asks of the scan's capacities.

    variant_per_block  per block, tasks with 1..16 keys and at least two keys off the task's most
                       common base: neither uniform_ref nor one_error_ref can settle them, so each
                       needs a queue record (blk_cap)
    listed_per_block   per block, called tasks that are not reference-only (1..32 keys, all on an
                       upper-case A/C/G/T reference base): each needs a list entry (list_cap); a
                       round above ROUND_KEYS lists its reference-only tasks too (not counted here)
    deep_tasks         tasks of more than 16 keys that are not reference-only: deep-list entries
    round_keys_max / round_keys_min
                       largest key total of an aligned round of ROUND_TASKS consecutive tasks of a
                       block / smallest of the rounds that hold ROUND_TASKS tasks of the batch
    first_key_off_max  largest offset of a not-reference-only task's first key inside its block
                       (the list entry adds the block's alignment, 0..7 keys, to it)"""
    ref = np.asarray(key_batch["ref"])
    L = len(ref)
    k = np.asarray(key_batch["k"]).reshape(-1).astype(np.int64)
    T = L * n
    keys = np.asarray(key_batch["keys"])
    nk = int(k.sum())
    assert nk == int(key_batch["block_off"][(L + SITE_BLOCK - 1) // SITE_BLOCK] - key_batch["block_off"][0])
    task = np.repeat(np.arange(T), k)
    cnt = np.bincount(task * 4 + (keys[:nk] & 3).astype(np.int64), minlength=T * 4).reshape(T, 4)
    rt = np.repeat(ref, n)
    called = (rt & 0x80) == 0
    refb = np.full(256, -1, np.int64)
    refb[REF_UPPER] = np.arange(4)
    rb = refb[rt]
    on_ref = cnt[np.arange(T), np.maximum(rb, 0)]
    ref_only = called & (rb >= 0) & (k >= 1) & (k <= FAST_MAX) & (on_ref == k)
    listed = called & ~ref_only
    variant = called & (k >= 1) & (k <= NET_MAX) & (k - cnt.max(axis=1) >= 2)
    deep = listed & (k > NET_MAX)
    nblk = (L + SITE_BLOCK - 1) // SITE_BLOCK
    bt = SITE_BLOCK * n

    def per_block(a):
        p = np.zeros(nblk * bt, np.int64)
        p[:T] = a
        return p.reshape(nblk, bt)
    kblk = per_block(k)
    rounds = (bt + ROUND_TASKS - 1) // ROUND_TASKS
    kr = np.zeros((nblk, rounds * ROUND_TASKS), np.int64)
    kr[:, :bt] = kblk
    rk = kr.reshape(nblk, rounds, ROUND_TASKS).sum(axis=2)
    real = np.zeros((nblk, rounds * ROUND_TASKS), np.int64)
    real[:, :bt] = per_block(np.ones(T, np.int64))
    whole = real.reshape(nblk, rounds, ROUND_TASKS).sum(axis=2) == ROUND_TASKS   # rounds of 128 tasks of the batch
    first = np.cumsum(kblk, axis=1) - kblk
    lb = per_block(listed)
    return {"variant_per_block": per_block(variant).sum(axis=1), "listed_per_block": lb.sum(axis=1),
            "deep_tasks": int(deep.sum()), "round_keys_max": int(rk.max()), "round_keys_min": int(rk[whole].min()),
            "first_key_off_max": int((first * lb).max())}


# ---- the routes
def _names(n):
    keep = [b"chr1", (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)]), (C.c_char_p * 2)(b"popA", b"popB")]
    return keep


def _oracle_nucdiv(params, batch, L, keep):
    lib = harness.oracle()
    c = harness.OrcCmd()
    c.cmd, c.output, c.min_sites, c.min_snps, c.min_freq = 4, 0, 10, 10, 1
    c.windowed, c.win_size, c.beg, c.end = 1, 10000, 0, L
    c.chr_name = keep[0]
    c.sample_names = C.cast(keep[1], C.POINTER(C.c_char_p))
    c.pop_names = C.cast(keep[2], C.POINTER(C.c_char_p))
    ref, dep = np.ascontiguousarray(batch["ref"]), np.ascontiguousarray(batch["depth"])
    rd = np.ascontiguousarray(batch["reads"])
    cap = 1 << 22
    buf = C.create_string_buffer(cap)
    r = lib.orc_run(C.byref(harness.oracle_params_from(params)), C.byref(c), L, ref.ctypes.data, dep.ctypes.data,
                    rd.ctypes.data, buf, cap)
    assert r >= 0
    return buf.value.decode()


def _stream_rows(ctx, kb, L, n, piece, compact, keep):
    """The host key batch `kb` pushed in pieces of `piece` positions: (rows, nucdiv text, pushes)."""
    from popbam_amd import _lib
    rb = ctx.row_bytes
    cmd = _lib.PbgCmd()
    cmd.cmd, cmd.output, cmd.min_sites, cmd.min_snps, cmd.min_freq = 4, 0, 10, 10, 1
    cmd.windowed, cmd.win_size, cmd.beg, cmd.end = 1, 10000, 0, L
    cmd.chr_name = keep[0]
    cmd.sample_names = C.cast(keep[1], C.POINTER(C.c_char_p))
    cmd.pop_names = C.cast(keep[2], C.POINTER(C.c_char_p))
    k2 = kb["k"].reshape(L, n)
    boff = kb["block_off"]
    host_rows = np.zeros(L * rb, np.uint8)
    pushes = 0
    with _lib.Stream(ctx, [cmd], 0, L) as st:
        for a in range(0, L, piece):
            b = min(L, a + piece)
            ref = np.ascontiguousarray(kb["ref"][a:b])
            kk = np.ascontiguousarray(k2[a:b])
            rq = np.ascontiguousarray(kb["rmsq"].reshape(L, n)[a:b])
            k0, k1 = int(boff[a // 64]), int(boff[(b + 63) // 64])
            keys = np.ascontiguousarray(kb["keys"][k0:k1]) if k1 > k0 else np.zeros(8, np.uint16)
            st.push(_lib.PbgPileup(b - a, a, ref.ctypes.data, kk.ctypes.data, rq.ctypes.data, None, keys.ctypes.data),
                    compact=compact)
            pushes += 1
        st.finish()
        st.rows_into(host_rows.ctypes.data, host_rows.size)
        text = st.text(0)
    return host_rows, text, pushes


def check_call_routes(ctx, params, batch, routes="abcd", piece=None, nucdiv=False, oracle=None, kb=None):
    """`batch` through the call pipeline, every route bitwise against orc_call_sites:
      a) rows only: pbg_call_sites(..., cb=NULL) on a device batch;
      b) consensus words: pbg_call_sites with cb -- the words of every task, and the rows;
      c) the stream: pbg_stream_* over the host key batch in pieces of whole 64-position blocks
         (`piece` positions; by default a third of the batch's blocks, so at least 3 pushes);
         nucdiv: its TSV against the oracle's main_nucdiv restatement (orc_run), too;
      d) the stream with compact pieces (feed.compact, pbg_stream_push_compact): rows.
    pbg_check is clean after each route.  `oracle` / `kb`: harness.oracle_call's and
    harness.key_batch's results when the caller has them.  Returns (counted positions, tasks
    whose rms fails min_rmsQ)."""
    import torch
    from popbam_amd import _lib, feed
    L = len(batch["ref"])
    n = params.n_samples
    rb = ctx.row_bytes
    ocb, types, _, flags = oracle if oracle is not None else harness.oracle_call(harness.oracle_params_from(params), batch)
    expect = harness.rows_from_oracle(types, flags, rb)
    if kb is None:
        kb = harness.key_batch(batch, params)
    if "a" in routes or "b" in routes:
        dev = {k: torch.from_numpy(np.ascontiguousarray(kb[k]).view(np.uint8).reshape(-1)).cuda()
               for k in ("ref", "k", "rmsq", "block_off", "keys")}
        if dev["keys"].numel() == 0:
            dev["keys"] = torch.zeros(16, dtype=torch.uint8, device="cuda")
        pl = _lib.PbgPileup(L, 0, *[dev[k].data_ptr() for k in ("ref", "k", "rmsq", "block_off", "keys")])
        rows = torch.zeros(L * rb + 16, dtype=torch.uint8, device="cuda")
        if "a" in routes:   # rows only
            ctx.check(ctx.lib.pbg_call_sites(ctx.h, C.byref(pl), rows.data_ptr(), None, None), "pbg_call_sites")
            ctx.sync_check()
            got = rows[:L * rb].cpu().numpy()
            bad = np.nonzero((got.reshape(L, rb) != expect.reshape(L, rb)).any(axis=1))[0]
            assert bad.size == 0, f"rows-only: {bad.size} rows differ, first at {bad[0]}"
        if "b" in routes:   # consensus words
            cb = torch.zeros(L * n, dtype=torch.int64, device="cuda")
            rows.zero_()
            ctx.check(ctx.lib.pbg_call_sites(ctx.h, C.byref(pl), rows.data_ptr(), cb.data_ptr(), None), "pbg_call_sites")
            ctx.sync_check()
            cbh = cb.cpu().numpy().view(np.uint64).reshape(L, n)
            bad = np.nonzero((cbh != ocb).any(axis=1))[0]
            assert bad.size == 0, f"words: {bad.size} positions differ, first {bad[0]}: gpu {cbh[bad[0]]} oracle {ocb[bad[0]]}"
            assert np.array_equal(rows[:L * rb].cpu().numpy(), expect)
            del cb
        del dev, rows
    keep = _names(n)
    nblk = (L + SITE_BLOCK - 1) // SITE_BLOCK
    min_pushes = 0
    if piece is None:
        piece, min_pushes = SITE_BLOCK * max(1, nblk // 3), min(3, nblk)
    if "c" in routes:   # streamed host batch
        host_rows, text, pushes = _stream_rows(ctx, kb, L, n, piece, False, keep)
        ctx.sync_check()
        assert pushes >= min_pushes
        bad = np.nonzero((host_rows.reshape(L, rb) != expect.reshape(L, rb)).any(axis=1))[0]
        assert bad.size == 0, f"stream: {bad.size} rows differ, first at {bad[0]}"
        if nucdiv:
            assert text == _oracle_nucdiv(params, batch, L, keep)
    if "d" in routes:   # streamed compact pieces
        assert params.max_depth <= 33025   # include/popbam_gpu.h pbg_stream_push_compact
        cmp = feed.compact(kb, n, ctx.k_bytes)
        host_rows, _, pushes = _stream_rows(ctx, cmp, L, n, piece, True, keep)
        ctx.sync_check()
        assert pushes >= min_pushes
        bad = np.nonzero((host_rows.reshape(L, rb) != expect.reshape(L, rb)).any(axis=1))[0]
        assert bad.size == 0, f"compact stream: {bad.size} rows differ, first at {bad[0]}"
    counted = int(((flags & 2) > 0).sum())
    failed_rms = int((((ocb >> np.uint64(48)) & np.uint64(0xFFFF)) < np.uint64(params.min_rmsQ)).sum())
    return counted, failed_rms


# ---- the named batches of test_call_edges.py
LADDER = np.array([1, 2, 3, 8, 9, 12, 13, 16, 17, 24, 25, 31, 32, 33, 34, 63, 64, 65, 127, 128, 254, 255])
LADDER_KINDS = np.array([0, 0, 0, 1, 2, 3, 4, 5])
LADDER16 = np.array([3, 17, 255, 256, 257, 300, 511, 512, 899, 900, 1000])
MIXED_DEEP = np.array([17, 32, 33, 100, 255])


def _lower_runs(L, rng, run=200):
    """Runs of `run` lower-case (1) or 'N' (2) positions, about every third run, the rest upper-case."""
    r = rng.integers(0, 6, (L + run - 1) // run)
    return np.repeat(np.where(r == 0, 1, np.where(r == 1, 2, 0)), run)[:L]


def _seed(name):
    return [0xC0FFEE30] + [ord(c) for c in name]


def _ladder(name, n, rng, variant):
    L = 64 * 40 + 17   # the last block partial
    # A depth-1 task off the reference mostly fails min_depth (clean_heterozygotes' arithmetic on the
    # packed word borrows from its read count) and a depth-1 read of mapQ 20 fails min_rmsQ, each
    # taking its whole position out of the count: above 64 samples depth 1 is drawn half as often,
    # which keeps more than a quarter of the positions counted (0.21 at 126 samples otherwise)
    w = np.where((LADDER == 1) & (n > 64), 0.5, 1.0)
    depth = rng.choice(LADDER, (L, n), p=w / w.sum())
    kind = LADDER_KINDS[rng.integers(0, LADDER_KINDS.size, (L, n))]
    lower = np.zeros(L, np.int64)
    if variant == "zero":    # k = 0 tasks
        depth = np.where(rng.random((L, n)) < 0.01, 0, depth)
    if variant == "lower":
        lower = _lower_runs(L, rng)
    batch = edge_batch(rng.integers(0, 4, L), lower, depth, kind, rng, illumina=variant == "flag02")
    if variant == "zero":    # whole positions without a callback (ref bit 7)
        batch["ref"][rng.random(L) < 0.03] |= 0x80
        batch["ref"][700:764] |= 0x80
    kw = {"flag20": dict(flag=0x20), "flag02": dict(flag=0x02), "snpq40": dict(min_snpQ=40)}.get(variant, {})
    return dict(min_depth=1, **kw), batch


def _ladder16(name, n, rng):
    L = 64 * 8
    depth = LADDER16[rng.integers(0, LADDER16.size, (L, n))]
    kind = LADDER_KINDS[rng.integers(0, LADDER_KINDS.size, (L, n))]
    return dict(min_depth=1, max_depth=900), edge_batch(rng.integers(0, 4, L), np.zeros(L, np.int64), depth, kind, rng,
                                                        max_depth=900)


def _capacity(name, n, rng, variant):
    L = 64 * 6 + 9
    lower = np.zeros(L, np.int64)
    kw = {}
    if variant in ("var", "var20", "varlow"):    # every task a real variant of 3..16 keys
        depth = rng.integers(3, 17, (L, n))
        kind = np.full((L, n), 3)
        if variant == "var20":
            kw = dict(flag=0x20)
        if variant == "varlow":                   # one lower-case run: the stream's mid-block settling
            lower[100:300] = 1
    elif variant == "mixed":
        # shallow reference / uniform tasks, and in every position one sample at depth 17 / 32 / 33 /
        # 100 / 255: sample 0 and sample n-1 at the first and at the last position of each block
        depth = rng.integers(3, 13, (L, n))
        kind = np.array([0, 0, 0, 1])[rng.integers(0, 4, (L, n))]
        smp = rng.integers(0, n, L)
        p = np.arange(L)
        blk = p // 64
        smp = np.where(p % 64 == 0, np.where(blk % 2 == 0, 0, n - 1), smp)
        smp = np.where(p % 64 == 63, np.where(blk % 2 == 0, n - 1, 0), smp)
        depth[p, smp] = MIXED_DEEP[rng.integers(0, MIXED_DEEP.size, L)]
        kind[p, smp] = LADDER_KINDS[rng.integers(0, LADDER_KINDS.size, L)]
    else:                                         # "alt": a block of depth 2..6, then one of depth 40..70
        deep_blk = ((np.arange(L) // 64) % 2 == 1)[:, None]
        depth = np.where(deep_blk, rng.integers(40, 71, (L, n)), rng.integers(2, 7, (L, n)))
        kind = LADDER_KINDS[rng.integers(0, LADDER_KINDS.size, (L, n))]
        kw = dict(min_depth=1)
    return kw, edge_batch(rng.integers(0, 4, L), lower, depth, kind, rng)


def _deep_list(name, n, rng, blocks):
    L = 64 * blocks
    depth = rng.integers(17, 25, (L, n))
    kind = np.array([1, 2, 3, 5])[rng.integers(0, 4, (L, n))]
    return {}, edge_batch(rng.integers(0, 4, L), np.zeros(L, np.int64), depth, kind, rng)


def _far_keys(name, n, rng):
    L = 64 * 2 + 5
    depth = rng.integers(250, 300, (L, n))
    kind = LADDER_KINDS[rng.integers(0, LADDER_KINDS.size, (L, n))]
    return dict(max_depth=300), edge_batch(rng.integers(0, 4, L), np.zeros(L, np.int64), depth, kind, rng)


class Case:
    """A named batch: params, the raw batch, its key batch (feed.pack) and its oracle results."""

    def __init__(self, name, n, kw, batch):
        from popbam_amd import workload
        self.name, self.n, self.batch = name, n, batch
        self.params = workload.default_params(n, 2, **kw)
        self.L = len(batch["ref"])
        self.kb = harness.key_batch(batch, self.params)
        self.oracle = harness.oracle_call(harness.oracle_params_from(self.params), batch)

    @property
    def counted(self):
        return (self.oracle[3] & 2) > 0

    def census(self):
        return census(self.kb, self.n)


@functools.lru_cache(maxsize=None)
def case(name):
    """family[-variant]-n, e.g. 'A-12', 'A-lower-24', 'A16-4', 'B-var-96', 'C-12', 'C300-12', 'D-126'."""
    parts = name.split("-")
    fam, n = parts[0], int(parts[-1])
    variant = parts[1] if len(parts) == 3 else ""
    rng = np.random.default_rng(_seed(name))
    if fam == "A":
        kw, batch = _ladder(name, n, rng, variant)
    elif fam == "A16":
        kw, batch = _ladder16(name, n, rng)
    elif fam == "B":
        kw, batch = _capacity(name, n, rng, variant)
    elif fam == "C":
        kw, batch = _deep_list(name, n, rng, 1500)
    elif fam == "C300":
        kw, batch = _deep_list(name, n, rng, 300)
    elif fam == "D":
        kw, batch = _far_keys(name, n, rng)
    else:
        raise KeyError(name)
    return Case(name, n, kw, batch)


def run_case(name, routes):
    """A case through `routes` on a fresh context (a context keeps the largest batch's queues)."""
    from popbam_amd import _lib
    c = case(name)
    ctx = _lib.Context(c.params, 0)
    try:
        return check_call_routes(ctx, c.params, c.batch, routes=routes, oracle=c.oracle, kb=c.kb)
    finally:
        ctx.close()
