"""bench.py's per-config defaults (CPU): configs[3] streams a whole 125 Mbp contig per chunk in
the serial pass (one ~64 GB key buffer) and 2^25 positions with --overlap (two buffers),
configs[4] 2^23 positions at 96 samples; an explicit --chunk is kept."""
import os
import sys

import pytest


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


@pytest.mark.parametrize("argv,chunk,samples", [
    ([], 1 << 25, 12),
    (["--config", "3"], 1 << 27, 24),
    (["--config", "3", "--overlap"], 1 << 25, 24),
    (["--config", "3", "--chunk", str(1 << 26)], 1 << 26, 24),
    (["--config", "3", "--chunk", str(1 << 25)], 1 << 25, 24),   # explicit 2^25 kept (was the argparse default)
    (["--config", "4", "--chunk", str(1 << 25)], 1 << 25, 96),
    (["--config", "4"], 1 << 23, 96),
])
def test_config_defaults(monkeypatch, argv, chunk, samples):
    a = _parse(argv, monkeypatch)
    assert a.chunk == chunk and a.samples == samples
    assert a.chunk % 64 == 0   # whole 64-position blocks (genome.GenomePass)
    if a.config == 3 and len(argv) == 2:
        assert a.chunk >= a.contig_len   # the default serial pass: one chunk per contig


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    a = _parse([], monkeypatch)
    assert a.full is False and a.dump_outputs is None
    a = _parse(["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full is True and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        _parse(["--steps", "0"], monkeypatch)


@pytest.mark.parametrize("n,k", [(10, 10), (10, 50), (11, 3), (1000, 7), (3_000_000_000, 1000)])
def test_spread_sample_is_fixed_ascending_and_distinct(n, k):
    import numpy as np

    import bench
    a, b = bench.spread_sample(n, k, 5), bench.spread_sample(n, k, 5)
    assert np.array_equal(a, b) and len(a) == min(n, k)
    assert a[0] >= 0 and a[-1] < n and np.all(np.diff(a) > 0)
    if k < n:
        assert not np.array_equal(a, bench.spread_sample(n, k, 6))


def test_dump_outputs_writes_every_field_and_samples_what_is_large(tmp_path, monkeypatch):
    """dump_outputs on host tensors: all windows and rows when they fit, else the same seeded
    sample of windows for every field (window_index) and of positions (rows_index); two window
    groups and two row regions are concatenated in order; ints convert exactly."""
    import numpy as np
    import torch

    import bench
    g = torch.Generator().manual_seed(1)
    groups = [(nw, {"num_sites": torch.randint(0, 1 << 30, (nw,), dtype=torch.int32, generator=g),
                    "pi": torch.rand(nw * 2, dtype=torch.float64, generator=g)}) for nw in (5, 8)]
    rows = [torch.randint(0, 256, (n * 4,), dtype=torch.uint8, generator=g) for n in (6, 9)]
    whole = {f: np.concatenate([t[f].numpy().reshape(nw, -1) for nw, t in groups]) for f in ("num_sites", "pi")}
    whole_rows = np.concatenate([r.numpy().reshape(-1, 4) for r in rows])

    def load(d):
        return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}

    info = bench.dump_outputs(str(tmp_path / "all"), torch, 7, ["num_sites", "pi"], groups, rows, 4)
    a = load(tmp_path / "all")
    assert sorted(a) == sorted(info["arrays"]) == ["num_sites", "pi", "rows", "rows_index", "window_index"]
    assert a["pi"].dtype == np.float64 and a["num_sites"].dtype == np.float64 and a["rows"].dtype == np.float32
    assert np.array_equal(a["num_sites"], whole["num_sites"]) and np.array_equal(a["pi"], whole["pi"])
    assert np.array_equal(a["rows"], whole_rows) and np.array_equal(a["rows_index"], np.arange(15))
    assert info["bytes"] == sum(v.nbytes for v in a.values())

    monkeypatch.setattr(bench, "DUMP_WINDOWS_BYTES", 8 * 3 * 4)   # room for 4 windows of 3 values
    monkeypatch.setattr(bench, "DUMP_ROWS_BYTES", 4 * 4 * 5)      # and 5 rows of 4 bytes
    bench.dump_outputs(str(tmp_path / "s1"), torch, 7, ["num_sites", "pi"], groups, rows, 4)
    bench.dump_outputs(str(tmp_path / "s2"), torch, 7, ["num_sites", "pi"], groups, rows, 4)
    s1, s2 = load(tmp_path / "s1"), load(tmp_path / "s2")
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
    wi, ri = s1["window_index"].astype(int), s1["rows_index"].astype(int)
    assert len(wi) == 4 and len(ri) == 5 and wi.max() >= 5 and ri.max() >= 6   # both groups / regions drawn from
    assert np.array_equal(s1["num_sites"], whole["num_sites"][wi]) and np.array_equal(s1["pi"], whole["pi"][wi])
    assert np.array_equal(s1["rows"], whole_rows[ri])


def test_traffic_split_bounds_the_hbm_share():
    """A counted traffic above what HBM can deliver in the launch's time is labelled as at least
    that excess served by the Infinity Cache (configs[3]'s 104.7 GB in 15.385 ms
    is 6.81 TB/s counted, above the 6.29 TB/s achievable)."""
    import bench
    s = bench.traffic_split(104_700_000_000, 15.385)
    assert s["counted_GBps"] > bench.HBM_ACHIEVABLE_GBS
    assert s["hbm_bytes_at_most"] == int(6290e9 * 15.385e-3)
    assert s["hbm_bytes_at_most"] + s["infinity_cache_bytes_at_least"] == 104_700_000_000
    s = bench.traffic_split(20_370_000_000, 3.4142)   # configs[2]: within what HBM can deliver
    assert s["infinity_cache_bytes_at_least"] == 0
    assert bench.traffic_split(None, 3.0) is None


@pytest.mark.parametrize("v", [0, 1, 2, 3, 16, 17, 18, 33, 181, 400])
def test_zns_chain_floor_counts_the_kernels_padded_adds(v):
    """window_stats.zns_chain: the longest chain's dependent adds as window_zns_kernel issues them
    (each row of pairs (a, a+1..V-1) padded to a multiple of 16: zns_rounds in stats_kernel.hip),
    against a direct count over the rows."""
    import torch

    import bench
    z = bench.zns_chain_floor(torch.tensor([3, v, 1], dtype=torch.int32))
    assert z["longest_chain_sites"] == max(v, 3)
    vv = max(v, 3)
    rows = [vv - 1 - a for a in range(vv - 1)]              # row a holds pairs (a, a+1 .. V-1)
    assert z["pairs"] == sum(rows)
    assert z["adds_padded"] == sum(-(-r // 16) * 16 for r in rows)
    assert z["floor_ms_at_7_cycles_2p4GHz"] == round(z["adds_padded"] * 7 / 2.4e9 * 1e3, 4)
