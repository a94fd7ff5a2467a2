"""Call-pipeline parity at the depth edges and at the queue / list capacity limits.

The synthetic workloads of the other call tests have mean depth 10 (per-sample depths up to about
30), where a block lists about 65 tasks and queues a handful; the one deep golden case sits near
depth 300 at 4 samples.  The batches here (call_edges.case) put tasks on both sides of every key
count at which call_kernel.hip takes another path, and past every fixed capacity that sends work
to a fallback path:

  A     depth ladder 1..255 (16 / 17: the 16-wire networks against the 32-wire network and the
        deep list; 32 / 33: kFastMax and call_sample_any; 254 / 255: the end of u8 k) with six read
        patterns per depth, at 12, 13, 24, 25, 64 and 126 samples (13: the first non-narrow
        instance, 24: the last with LDS info bytes, 25: HBM info bytes and the 448-entry list),
        with flags 0x20 and 0x02, min_snpQ 40, k = 0 tasks and positions without a callback, and
        runs of a lower-case / N reference (the stream's mid-block settling scan instance)
  A16   u16 k: depths 3..900 around 255 / 256 and 511 / 512 at max_depth 900
  B     capacity: every task a variant of 3..16 keys (more queue records than a block's region
        holds, more listed tasks than the wave's list: the overflow kernel; with a lower-case run,
        the mid-block settling); one deep sample per position among shallow ones, at the first and
        last sample of a block's first and last position; blocks alternating between rounds far
        below and far above the 4,096 keys a round may stage
  C     more deep tasks than the deep list holds
  D     tasks whose keys start 2^21 or more keys into their block
  E     A, B, D and a cut of C on the PBG_BOUNDS build: no key load outside the batch and no store
        outside its array on any of these paths

The CPU tests show that each batch is what it claims to be (call_edges.census against the limits
restated from the source; the oracle counts enough positions, rows being zero elsewhere) before
the GPU tests compare anything; the GPU tests run each batch through the routes of
call_edges.check_call_routes, bitwise against orc_call_sites."""
import os
import subprocess
import sys

import numpy as np
import pytest

import call_edges as ce

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LIB = os.path.join(REPO, "popbam_amd", "variants", "bounds", "libpopbam_gpu.so")

A_CASES = ["A-12", "A-13", "A-24", "A-25", "A-64", "A-126", "A-flag20-12", "A-flag02-12", "A-snpq40-12",
           "A-zero-13", "A-zero-25", "A-lower-12", "A-lower-24", "A-lower-25"]
A16_CASES = ["A16-4", "A16-12"]
B_N = [12, 24, 25, 96]
B_VAR = [f"B-{v}-{n}" for n in B_N for v in ("var", "var20", "varlow")]
B_MIXED = [f"B-mixed-{n}" for n in B_N]
B_ALT = [f"B-alt-{n}" for n in B_N]
E_CASES = ["A-12", "A-25", "B-var-12", "B-var-96", "D-126", "C300-12"]
ALL_CASES = A_CASES + A16_CASES + B_VAR + B_MIXED + B_ALT + ["C-12", "C300-12", "D-126"]


# ---------------------------------------------------------------- CPU: the batches are what they claim
@pytest.mark.parametrize("name", ALL_CASES)
def test_pack_gives_k_equal_depth_and_a_quarter_counted(name):
    c = ce.case(name)
    dep = c.batch["depth"]
    assert dep.max() <= c.params.max_depth
    assert np.array_equal(c.kb["k"].astype(np.int64), dep.astype(np.int64))
    share = c.counted.mean()
    print(f"{name}: {c.L} positions, {int(dep.sum(dtype=np.int64))} keys, counted share {share:.2f}")
    assert share >= 0.25


def test_u16_ladder_reaches_its_cap():
    for name in A16_CASES:
        k = ce.case(name).kb["k"]
        assert k.dtype == np.uint16 and k.max() == 900 and (k == 899).any() and (k == 256).any() and (k == 255).any()


@pytest.mark.parametrize("name", A_CASES)
def test_ladder_cells_are_filled_at_counted_positions(name):
    """Every (depth edge, kind) cell has tasks at positions the oracle counts: elsewhere the row is
    zero whatever the task's call."""
    c = ce.case(name)
    cnt = np.broadcast_to(c.counted[:, None], c.batch["depth"].shape)
    dep, kind = c.batch["depth"][cnt].astype(np.int64), c.batch["kind"][cnt]
    cells = np.bincount(dep * 8 + kind, minlength=256 * 8).reshape(256, 8)[ce.LADDER][:, :6]
    print(f"{name}: smallest (depth, kind) cell {cells.min()} tasks, counted share {c.counted.mean():.2f}")
    assert cells.min() >= 8
    # the single read of kinds 2 and 5 at key 0 and at key 1 (the list pass's majority-base rule)
    kb = c.kb
    k = kb["k"].reshape(-1).astype(np.int64)
    first = np.cumsum(k) - k
    base = (kb["keys"] & 3).astype(np.int64)
    t = np.nonzero((c.batch["kind"].reshape(-1) == 2) & (k >= 3) & (k <= 16) & np.repeat(c.counted, c.n))[0]
    b0, b1, b2 = base[first[t]], base[first[t] + 1], base[first[t] + 2]
    assert ((b0 != b1) & (b1 == b2)).sum() >= 8 and ((b0 != b1) & (b0 == b2)).sum() >= 8


def test_ladder_variants_hold_what_they_add():
    for name in ("A-zero-13", "A-zero-25"):
        c = ce.case(name)
        nocb = (c.batch["ref"] & 0x80) > 0
        assert nocb[700:764].all() and 100 < nocb.sum() < c.L // 4
        assert ((c.kb["k"] == 0) & ~nocb[:, None]).sum() >= 100
    for name in ("A-lower-12", "A-lower-24", "A-lower-25"):
        ref = ce.case(name).batch["ref"]
        low = np.isin(ref, np.frombuffer(b"acgt", np.uint8))
        assert low[:-1][np.diff(low.astype(int)) != 0].size >= 2 and low.sum() >= 200 and (ref == ord("N")).sum() >= 200


@pytest.mark.parametrize("name", B_VAR)
def test_variant_blocks_exceed_queue_region_and_list(name):
    c = ce.case(name)
    s = c.census()
    full = c.L // 64   # the whole blocks
    print(f"{name}: variant tasks per block {s['variant_per_block'][:full].min()}..{s['variant_per_block'].max()} "
          f"(queue region {ce.blk_cap(c.n)}), listed per block {s['listed_per_block'][:full].min()} (list {ce.list_cap(c.n)})")
    assert s["variant_per_block"][:full].min() > ce.blk_cap(c.n)
    assert s["listed_per_block"][:full].min() > ce.list_cap(c.n)


@pytest.mark.parametrize("name", B_MIXED)
def test_mixed_blocks_place_the_deep_sample_at_the_corners(name):
    c = ce.case(name)
    k = c.kb["k"].astype(np.int64)
    assert ((k > 16).sum(axis=1) == 1).all()
    for b in range(c.L // 64):
        i, j = (0, c.n - 1) if b % 2 == 0 else (c.n - 1, 0)
        assert k[64 * b, i] > 16 and k[64 * b + 63, j] > 16
    deep = k[k > 16]
    assert all((deep == d).any() for d in ce.MIXED_DEEP)
    s = c.census()
    print(f"{name}: deep tasks {s['deep_tasks']}, listed per block {s['listed_per_block'].min()}..{s['listed_per_block'].max()}")
    assert s["deep_tasks"] >= c.L // 2


@pytest.mark.parametrize("name", B_ALT)
def test_alternating_blocks_cross_the_round_limit_both_ways(name):
    s = ce.case(name).census()
    print(f"{name}: round keys {s['round_keys_min']}..{s['round_keys_max']} (limit {ce.ROUND_KEYS})")
    assert s["round_keys_max"] > ce.ROUND_KEYS and 0 < s["round_keys_min"] < ce.ROUND_KEYS


@pytest.mark.parametrize("name", ["C-12", "C300-12"])
def test_deep_tasks_exceed_the_deep_list(name):
    c = ce.case(name)
    s = c.census()
    print(f"{name}: deep tasks {s['deep_tasks']} (deep list {ce.task_cap(c.L, c.n)})")
    assert ce.task_cap(c.L, c.n) == {"C-12": 264_000, "C300-12": 72_736}[name]
    assert s["deep_tasks"] > ce.task_cap(c.L, c.n)


def test_far_keys_start_past_the_list_offset():
    c = ce.case("D-126")
    s = c.census()
    print(f"D-126: largest first-key offset in a block {s['first_key_off_max']} (limit {ce.LIST_OFF_MAX})")
    assert s["first_key_off_max"] >= ce.LIST_OFF_MAX
    assert c.kb["k"].dtype == np.uint16 and c.kb["k"].max() > 255


# ---------------------------------------------------------------- GPU: every route against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("name", A_CASES + A16_CASES)
def test_depth_ladder_matches_oracle(gpu_lib, name):
    ce.run_case(name, "abcd")


@pytest.mark.gpu
@pytest.mark.parametrize("name", B_VAR + B_MIXED + B_ALT)
def test_capacity_batches_match_oracle(gpu_lib, name):
    ce.run_case(name, "abcd")


@pytest.mark.gpu
def test_deep_list_overflow_matches_oracle(gpu_lib):
    ce.run_case("C-12", "ab")


@pytest.mark.gpu
def test_far_keys_match_oracle(gpu_lib):
    ce.run_case("D-126", "abc")


# ---------------------------------------------------------------- GPU: the same paths on the bounds build
SNIPPET = r"""
import sys
sys.path[:0] = [{repo!r}, {tests!r}]
import call_edges as ce
from popbam_amd import _lib
assert _lib.load().pbg_build_info() == b"bounds"
out = []
for name in {names!r}:
    try:
        ce.run_case(name, "ab")   # rows and words equal the oracle's; pbg_check returns 0
        out.append(name + ":ok")
    except (AssertionError, RuntimeError) as e:
        out.append(name + ":" + type(e).__name__ + " " + str(e)[:200].replace("\n", " ").replace("|", "/"))
print("|".join(out))
"""


@pytest.mark.gpu
def test_edges_on_the_bounds_build(gpu_lib):
    """Rows-only and consensus-word calls of the edge batches on the PBG_BOUNDS build (a child
    process with POPBAM_GPU_LIB, as test_bounds_build._run): equal to the oracle, and pbg_check
    returns 0 -- no key load outside the batch, no store outside its array on the fallback paths."""
    assert os.path.exists(BOUNDS_LIB), "build it with __graft_entry__.build() (make bounds)"
    env = dict(os.environ)
    env.pop("PBG_BOUNDS_SELFTEST", None)
    env["POPBAM_GPU_LIB"] = BOUNDS_LIB
    code = SNIPPET.format(repo=REPO, tests=os.path.join(REPO, "tests"), names=E_CASES)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip().splitlines()[-1].split("|") == [n + ":ok" for n in E_CASES]
