"""The claim hand-out of the 4096-point c32 streaming kernel (fft_persist.hip.h, PersistClaim): the first rows of a batch are walked
with the grid's stride, the last ones are claimed one by one through two counters the context owns, which every launch leaves at zero.

Which workgroup computes a row must not show: every row of every call is compared bit for bit with the oracle, forward and inverse, in
place and out of place, through the C ABI, with guard bands (tests/redzone.py) round every buffer -- a claimed row written past the batch
damages a band, a row transformed twice (in place) or never (out of place: the band pattern stays) differs from the oracle.

Shapes: the persistent route starts at num_cus * 4 = 1024 rows; the grid is num_cus * 2 = 512 workgroups of one row each.  1024 / 1025 /
1537 / 2047 / 2049 rows put the seam between walked and claimed rows at, right behind, in the middle of and right in front of a whole
round of the grid.  kofft_hip_set_persist_claim_pct(100) claims everything (no walked row: the first row too is claimed), (0) leaves
only the rows the grid's stride does not cover -- one row at 1025, none at 1024 (every workgroup's single claim fails)."""
import ctypes as C

import numpy as np
import pytest

from conftest import rand_c, seeded
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu

N = 4096
ROWS = 2049  # the largest batch below
BATCHES = (1024, 1025, 1537, 2047, 2049)
FORMS = [(inverse, in_place) for inverse in (False, True) for in_place in (False, True)]


@pytest.fixture(scope="module")
def ref(oracle):
    """One seeded batch and its forward and inverse transforms, computed once; the tests use its first rows and leave it unchanged."""
    x = rand_c(seeded(0xC1A1), (ROWS, N), np.complex64)
    want = {False: oracle.fft_mt(x), True: oracle.fft_mt(x, inverse=True)}
    for a in (x, want[False], want[True]):
        a.setflags(write=False)
    return x, want


class Ctx:
    """A context of its own (the knobs are read when it is created)."""

    def __init__(self, lib, claim_pct=None):
        self.lib, self.ctx = lib, C.c_void_p()
        assert lib.kofft_hip_create(0, C.byref(self.ctx)) == 0
        if claim_pct is not None:
            assert lib.kofft_hip_set_persist_claim_pct(self.ctx, claim_pct) == 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        assert self.lib.kofft_hip_destroy(self.ctx) == 0

    def launch(self, arena, x, batch, inverse, in_place, name=""):
        """Enqueue one transform of x[:batch] in regions of `arena`; returns the region that will hold the result."""
        if in_place:
            buf = arena.inout(x[:batch], row_bytes=8 * N, name=f"inout{name}")
            return buf, lambda: self.lib.kofft_hip_fft_c32_dev(self.ctx, C.c_void_p(buf.addr), N, batch, int(inverse))
        src = arena.input(x[:batch], row_bytes=8 * N, name=f"in{name}")
        dst = arena.output(8 * N * batch, row_bytes=8 * N, name=f"out{name}")
        return dst, lambda: self.lib.kofft_hip_fft_c32_dev_oop(self.ctx, C.c_void_p(src.addr), C.c_void_p(dst.addr), N, batch, int(inverse))


def check_one(ctx, ref, batch, inverse, in_place, what):
    x, want = ref
    what = f"{what}: batch {batch} {'inverse' if inverse else 'forward'} {'in place' if in_place else 'out of place'}"
    arena = Arena("cuda", what)
    region, call = ctx.launch(arena, x, batch, inverse, in_place)
    assert call() == 0
    arena.verify()
    assert_rows_equal(arena.read(region, np.complex64, (batch, N)), want[inverse][:batch], what)


@pytest.mark.parametrize("batch", BATCHES)
def test_every_row_matches_the_oracle_at_the_measured_share(hiplib, ref, batch):
    with Ctx(hiplib) as ctx:
        for inverse, in_place in FORMS:
            check_one(ctx, ref, batch, inverse, in_place, "default share")


@pytest.mark.parametrize("pct,batch", [(100, 1024), (100, 1537), (0, 1025), (0, 1024), (50, 2049)],
                         ids=["all-claimed-1024", "all-claimed-1537", "one-claimed-row", "no-claimed-row", "half-2049"])
def test_split_at_zero_single_claimed_unit_and_no_claimed_row(hiplib, ref, pct, batch):
    with Ctx(hiplib, pct) as ctx:
        for inverse, in_place in FORMS:
            check_one(ctx, ref, batch, inverse, in_place, f"claim share {pct} %")


def test_a_share_above_100_is_refused(hiplib):
    with Ctx(hiplib) as ctx:
        assert hiplib.kofft_hip_set_persist_claim_pct(ctx.ctx, 101) == 6  # INVALID_VALUE
        assert hiplib.kofft_hip_set_persist_claim_pct(ctx.ctx, -1) == 0  # back to the default
        assert hiplib.kofft_hip_set_persist_claim_pct(None, 10) == -3    # KOFFT_ERR_NULL


@pytest.mark.parametrize("grid_pct", ["37", "71"])  # 189 and 363 workgroups on 256 CUs: neither divides 1537 or 2049
def test_grids_that_do_not_divide_the_batch(hiplib, ref, monkeypatch, grid_pct):
    monkeypatch.setenv("KOFFT_HIP_PERSIST_GRID_PCT", grid_pct)
    with Ctx(hiplib) as ctx:
        for batch in (1537, 2049):
            for inverse, in_place in FORMS:
                check_one(ctx, ref, batch, inverse, in_place, f"grid {grid_pct} %")
    with Ctx(hiplib, 100) as ctx:
        check_one(ctx, ref, 2049, False, True, f"grid {grid_pct} %, all claimed")


def test_counters_reset_themselves_between_back_to_back_launches(hiplib, ref):
    """Six launches on one context with no synchronisation in between, two batch sizes in turn: each starts from the zeros its predecessor
    left (a stale claim counter would skip rows -- band pattern in the output -- and a stale arrival counter would never reset them)."""
    x, want = ref
    with Ctx(hiplib) as ctx:
        arena = Arena("cuda", "six launches back to back")
        plan = [(1025 if i % 2 == 0 else 2049, i % 3 == 2, i % 2 == 1) for i in range(6)]
        calls = [ctx.launch(arena, x, b, inv, inp, name=str(i)) for i, (b, inv, inp) in enumerate(plan)]
        for region, _ in calls:
            region.addr  # lays the arena out (and synchronises) before the first launch
        for _, call in calls:
            assert call() == 0
        arena.verify()
        for i, ((region, _), (b, inv, inp)) in enumerate(zip(calls, plan)):
            assert_rows_equal(arena.read(region, np.complex64, (b, N)), want[inv][:b], f"launch {i} of six: batch {b} inverse {inv} in place {inp}")


def test_two_contexts_used_alternately_keep_their_own_counters(hiplib, ref):
    x, want = ref
    with Ctx(hiplib) as a, Ctx(hiplib) as b:
        arena = Arena("cuda", "two contexts in turn")
        plan = [(a, 1537, False, True), (b, 1025, False, False), (a, 1025, True, False), (b, 2049, False, True), (a, 2047, False, False),
                (b, 1537, True, True)]
        calls = [c.launch(arena, x, n, inv, inp, name=str(i)) for i, (c, n, inv, inp) in enumerate(plan)]
        for region, _ in calls:
            region.addr
        for _, call in calls:
            assert call() == 0
        arena.verify()
        for i, ((region, _), (_, n, inv, inp)) in enumerate(zip(calls, plan)):
            assert_rows_equal(arena.read(region, np.complex64, (n, N)), want[inv][:n], f"call {i}: batch {n} inverse {inv} in place {inp}")
