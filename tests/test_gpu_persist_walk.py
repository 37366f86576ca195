"""The direction and the kept zone of the 4096-point c32 streaming kernel's batch walk (fft_persist.hip.h, PersistClaim::mirror and
keep_from; kofft_amd/csrc/persist_walk.h): the kernel hands out walk indices, the memory row of index w is w or batch - 1 - w, and the
rows from keep_from on are stored with the default cache policy.  Under mode -1 a call on the buffer the previous call wrote walks the
other way.

Which way a batch was walked must not show: every row of every call is compared bit for bit with the oracle, forward and inverse, in
place and out of place, through the C ABI, with guard bands round every buffer -- a mirrored row computed from batch instead of batch - 1
lands in a band, a row taken twice shows in place, a row never taken leaves the band pattern out of place.  After every case the nine
claim words are read back and must be zero.

Shapes as in test_gpu_persist_claim.py: the persistent route starts at 1024 rows, the grid is 512 workgroups of one row each, so at the
default share every row of these batches is claimed; shares 0 and 50 put walked rows in front of them."""
import ctypes as C

import numpy as np
import pytest

from redzone import Arena
from rowcheck import assert_rows_equal
from test_gpu_persist_claim import FORMS, N, Ctx, check_one, ref  # noqa: F401  (ref: the module-scoped fixture, one oracle run)
from test_gpu_persist_rowmap import assert_counters_zero

pytestmark = pytest.mark.gpu

ROW = 8 * N
MIB = 1 << 20


class WalkCtx(Ctx):
    def __init__(self, lib, mode=None, keep_bytes=None, claim_pct=None):
        super().__init__(lib, claim_pct)
        if mode is not None:
            assert lib.kofft_hip_set_persist_walk(self.ctx, mode) == 0
        if keep_bytes is not None:
            assert lib.kofft_hip_set_persist_keep_bytes(self.ctx, keep_bytes) == 0

    def walk(self):
        """(launches so far, the last one mirrored, its keep_from, its batch): host-side state, no synchronisation."""
        words = (C.c_ulonglong * 4)()
        assert self.lib.kofft_hip_persist_walk_debug(self.ctx, words) == 0
        return tuple(int(w) for w in words)


def forced_keep_from(batch, keep_bytes):
    """persist_keep_from(..., clamp = true): modes 1 and 2."""
    rows = keep_bytes // ROW
    return batch if rows == 0 else max(0, batch - rows)


def run_forms(hiplib, ref, ctx, batch, mode, keep_bytes, what):
    for inverse, in_place in FORMS:
        check_one(ctx, ref, batch, inverse, in_place, what)
        launches, mirrored, keep_from, last_batch = ctx.walk()
        assert last_batch == batch and mirrored == (1 if mode == 2 else 0), what
        assert keep_from == (batch if mode == 0 else forced_keep_from(batch, keep_bytes)), what
    assert_counters_zero(hiplib, ctx, what)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("batch", [1024, 1025, 1537, 2049])
def test_every_row_matches_the_oracle_in_both_directions(hiplib, ref, batch, mode):
    with WalkCtx(hiplib, mode, MIB) as ctx:
        run_forms(hiplib, ref, ctx, batch, mode, MIB, f"walk mode {mode}, 1 MiB kept")


# batch 2049 at a share of 50 percent: rows [0, 1024) are walked, [1024, 2049) claimed in pieces of 512 and 513.  Kept zones: none; 32
# rows inside the last piece; exactly the claimed part; one row more (the last walked row too); the whole batch and more than it.
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("keep_rows", [0, 32, 1025, 1026, 2049, 5000], ids=lambda r: f"keep{r}")
def test_kept_zones_at_every_seam(hiplib, ref, keep_rows, mode):
    with WalkCtx(hiplib, mode, keep_rows * ROW, 50) as ctx:
        run_forms(hiplib, ref, ctx, 2049, mode, keep_rows * ROW, f"walk mode {mode}, {keep_rows} rows kept, share 50 %")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("pct", [0, 87, 100])
def test_claim_shares_in_both_directions(hiplib, ref, pct, mode):
    with WalkCtx(hiplib, mode, MIB, pct) as ctx:
        for batch in (1025, 1537):
            run_forms(hiplib, ref, ctx, batch, mode, MIB, f"walk mode {mode}, share {pct} %")


def test_an_odd_grid(hiplib, ref, monkeypatch):
    monkeypatch.setenv("KOFFT_HIP_PERSIST_GRID_PCT", "37")  # 189 workgroups on 256 CUs
    for mode, pct in ((2, None), (2, 50), (1, 50)):
        with WalkCtx(hiplib, mode, MIB, pct) as ctx:
            for batch in (1537, 2049):
                run_forms(hiplib, ref, ctx, batch, mode, MIB, f"grid 37 %, walk mode {mode}, share {pct}")


def test_the_setters_take_effect_at_the_next_launch_and_refuse_what_they_must(hiplib, ref):
    with WalkCtx(hiplib) as ctx:
        assert hiplib.kofft_hip_set_persist_walk(ctx.ctx, 2) == 0
        assert hiplib.kofft_hip_set_persist_keep_bytes(ctx.ctx, 3 * MIB) == 0
        run_forms(hiplib, ref, ctx, 1025, 2, 3 * MIB, "mode and zone set after creation")
        assert hiplib.kofft_hip_set_persist_walk(ctx.ctx, 3) == 6   # INVALID_VALUE
        assert hiplib.kofft_hip_set_persist_walk(ctx.ctx, -2) == 6
        assert hiplib.kofft_hip_persist_walk_debug(ctx.ctx, None) == -3  # KOFFT_ERR_NULL
    assert hiplib.kofft_hip_set_persist_walk(None, 0) == -3
    assert hiplib.kofft_hip_set_persist_keep_bytes(None, 0) == -3
    assert hiplib.kofft_hip_persist_walk_debug(None, (C.c_ulonglong * 4)()) == -3


class Rule:
    """persist_walk_rule and the record, restated: mirrored relative to the record when the input or the output range is exactly the
    range the last call wrote, ascending otherwise."""

    def __init__(self):
        self.last = None  # (address, bytes, mirrored)

    def next(self, src, dst, nbytes):
        follows = self.last is not None and self.last[:2] in ((src, nbytes), (dst, nbytes))
        mirrored = (not self.last[2]) if follows else False
        self.last = (dst, nbytes, mirrored)
        return mirrored


def test_six_calls_back_to_back_follow_the_rule(hiplib, oracle, ref):
    """Mode -1, no synchronisation between the calls: one buffer three times (ascending, descending, ascending), another buffer
    (ascending), out of place from that buffer into a third (descending: its input is what the call before wrote), then a longer batch
    on the first buffer (ascending: the size changed, and the record names the third buffer).  The direction of every call is read from
    the context right behind it and compared with the rule; the buffers are compared with the oracle's chain of the same transforms."""
    x, want = ref
    b1, b2 = 1025, 1537
    keep = 2 * MIB  # 64 rows: on for both batches under the rule (at most half the batch)
    with WalkCtx(hiplib, -1, keep) as ctx:
        arena = Arena("cuda", "six calls under the rule")
        a = arena.inout(x[:b2], row_bytes=ROW, name="a")
        b = arena.inout(x[:b1], row_bytes=ROW, name="b")
        c = arena.output(ROW * b1, row_bytes=ROW, name="c")
        lib, h = hiplib, ctx.ctx
        inplace = lambda r, n, inv: lib.kofft_hip_fft_c32_dev(h, C.c_void_p(r.addr), N, n, int(inv))  # noqa: E731
        plan = [(a, a, b1, False), (a, a, b1, True), (a, a, b1, False), (b, b, b1, False), (b, c, b1, False), (a, a, b2, False)]
        a.addr  # lays the arena out (and synchronises) before the first launch
        rule, took, expect = Rule(), [], []
        for i, (src, dst, n, inv) in enumerate(plan):
            if src is dst:
                assert inplace(dst, n, inv) == 0
            else:
                assert lib.kofft_hip_fft_c32_dev_oop(h, C.c_void_p(src.addr), C.c_void_p(dst.addr), N, n, int(inv)) == 0
            launches, mirrored, keep_from, last_batch = ctx.walk()
            assert launches == i + 1 and last_batch == n and keep_from == n - keep // ROW
            took.append(bool(mirrored))
            expect.append(rule.next(src.addr, dst.addr, n * ROW))
        assert took == expect == [False, True, False, False, True, False]
        arena.verify()
        back = oracle.fft_mt(want[False][:b1], inverse=True)  # a after two calls
        third = oracle.fft_mt(back)                            # a after three
        a_want = np.concatenate([oracle.fft_mt(third), want[False][b1:b2]])
        assert_rows_equal(arena.read(a, np.complex64, (b2, N)), a_want, "first buffer: three calls, then the longer batch")
        assert_rows_equal(arena.read(b, np.complex64, (b1, N)), want[False][:b1], "second buffer: one call, then read by the fifth")
        assert_rows_equal(arena.read(c, np.complex64, (b1, N)), oracle.fft_mt(want[False][:b1]), "third buffer: the fifth call's output")
        assert_counters_zero(hiplib, ctx, "six calls under the rule")
