"""The sharded claim hand-out of the 4096-point c32 streaming kernel (fft_persist.hip.h, PersistClaim): the claimed rows are cut into
contiguous pieces, each with a claim word of its own (two of them: the count that measured fastest; the context has room for eight); a
workgroup starts at shard blockIdx % shards and walks on to the next shard when a claim fails.  The word in the ninth line counts arrivals,
and the last workgroup to arrive zeroes every word the kernel uses.

(The row-to-workgroup maps this file was named for were measured in a copy model -- tools/ubench_copy4.hip, profiles/r08_copy_footprint.txt
-- and not built: none of them left the box's spread.  What is tested here is the part that was built.)

Every row of every call is compared bit for bit with the oracle, forward and inverse, in place and out of place, through the C ABI, with
guard bands round every buffer: a row claimed twice shows in place, a row never claimed leaves the band pattern out of place, a claim
beyond its shard's end either repeats a row or writes past the batch.  After every case the nine words are read back and must be zero.

Shapes as in test_gpu_persist_claim.py: the persistent route starts at 1024 rows, the grid is 512 workgroups of one row each."""
import ctypes as C

import numpy as np
import pytest

from redzone import Arena
from rowcheck import assert_rows_equal
from test_gpu_persist_claim import FORMS, N, Ctx, check_one, ref  # noqa: F401  (ref: the module-scoped fixture, one oracle run)

pytestmark = pytest.mark.gpu


def assert_counters_zero(hiplib, ctx, what):
    words = (C.c_uint * 9)(*([0xDEAD] * 9))
    assert hiplib.kofft_hip_persist_claim_debug(ctx.ctx, words) == 0
    assert list(words) == [0] * 9, f"{what}: claim words after the launch {list(words)}"


# pct = 0 claims only what the grid's stride leaves over: batch - 1024 units.  The pieces are floor(units / shards) long and the last one
# takes the remainder.  0 units: every shard is empty from the start; 1: all in the last shard, the others empty from the start (7: the
# same with eight shards); 8: even pieces; 7, 9 and 513: the last piece is one longer.
@pytest.mark.parametrize("batch,units", [(1024, 0), (1025, 1), (1031, 7), (1032, 8), (1033, 9), (1537, 513)])
def test_shards_that_are_empty_or_uneven(hiplib, ref, batch, units):
    assert batch - 1024 == units
    with Ctx(hiplib, 0) as ctx:
        for inverse, in_place in FORMS:
            check_one(ctx, ref, batch, inverse, in_place, f"{units} claimed units")
        assert_counters_zero(hiplib, ctx, f"{units} claimed units")


@pytest.mark.parametrize("pct,batch", [(100, 1024), (100, 1537), (100, 2049), (50, 2049), (87, 2047)])
def test_large_shares_over_the_shards(hiplib, ref, pct, batch):
    with Ctx(hiplib, pct) as ctx:
        for inverse, in_place in FORMS:
            check_one(ctx, ref, batch, inverse, in_place, f"claim share {pct} %")
        assert_counters_zero(hiplib, ctx, f"claim share {pct} %, batch {batch}")


# 189, 363 and 71 workgroups on 256 CUs (odd, and 71 = 7 mod 8): the shards start with unevenly many workgroups
@pytest.mark.parametrize("grid_pct", ["37", "71", "14"])
def test_grids_that_are_no_multiple_of_eight(hiplib, ref, monkeypatch, grid_pct):
    monkeypatch.setenv("KOFFT_HIP_PERSIST_GRID_PCT", grid_pct)
    for pct in (None, 100):
        with Ctx(hiplib, pct) as ctx:
            for batch in (1537, 2049):
                for inverse, in_place in FORMS:
                    check_one(ctx, ref, batch, inverse, in_place, f"grid {grid_pct} %, share {pct}")
            assert_counters_zero(hiplib, ctx, f"grid {grid_pct} %, share {pct}")


def test_nine_words_are_zero_after_back_to_back_launches_on_two_contexts(hiplib, ref):
    """Six launches on each of two contexts, the contexts in turn, no synchronisation in between, batches 1025 and 2049 in turn and the
    share changed between launches (the setter takes effect at the next launch): each launch starts from the zeros its predecessor left."""
    x, want = ref
    with Ctx(hiplib) as a, Ctx(hiplib) as b:
        arena = Arena("cuda", "twelve launches back to back")
        plan = [((a, b)[i % 2], 1025 if (i // 2) % 2 == 0 else 2049, i % 3 == 2, i % 4 >= 2, (-1, 100, 0)[(i // 2) % 3]) for i in range(12)]
        calls = [c.launch(arena, x, n, inv, inp, name=str(i)) for i, (c, n, inv, inp, _) in enumerate(plan)]
        for region, _ in calls:
            region.addr  # lays the arena out (and synchronises) before the first launch
        for (_, call), (c, _, _, _, pct) in zip(calls, plan):
            assert hiplib.kofft_hip_set_persist_claim_pct(c.ctx, pct) == 0
            assert call() == 0
        arena.verify()
        for i, ((region, _), (_, n, inv, inp, pct)) in enumerate(zip(calls, plan)):
            assert_rows_equal(arena.read(region, np.complex64, (n, N)), want[inv][:n], f"launch {i} of twelve: batch {n} inverse {inv} in place {inp} share {pct}")
        assert_counters_zero(hiplib, a, "first context")
        assert_counters_zero(hiplib, b, "second context")


def test_the_debug_accessor_refuses_null(hiplib):
    words = (C.c_uint * 9)()
    assert hiplib.kofft_hip_persist_claim_debug(None, words) == -3  # KOFFT_ERR_NULL
    with Ctx(hiplib) as ctx:
        assert hiplib.kofft_hip_persist_claim_debug(ctx.ctx, None) == -3
