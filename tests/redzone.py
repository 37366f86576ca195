"""Guard bands around every buffer of a call: one contiguous byte arena per case, laid out as

    band | region | band | band | region | band | ... | band

so that a store outside an output, or any store to an input, is seen after the call -- the job GPU AddressSanitizer would do where it
can run.  The arena is a torch uint8 tensor on a device ("cuda" in the GPU tests, "cpu" in this helper's own test) or, with
device="host", a numpy array for the host-pointer entry points.

    arena = Arena("cuda", "fft_c32_dev_oop n=4096 batch=257")
    x = arena.input(array, row_bytes=8 * n)              # uploaded, snapshot kept: must be unchanged after the call
    y = arena.output(nbytes, row_bytes=8 * n)            # pre-filled with the band pattern (or with `prefill`)
    call(x.addr, y.addr, ...)                            # the first .addr lays the arena out and allocates it: no region after that
    arena.verify()                                       # AssertionError naming case, region, side, offsets, length (in rows too)
    got = arena.read(y, np.complex64, (batch, n))

Band pattern: the 32-bit word 0x7FF8A5A5 repeated.  Read as f32 it is a NaN and so is a pair of them read as f64, so an over-read that
reaches a result turns it into NaN (the oracle comparison of the test then fails); it is neither the host's canonical NaN (0x7FC00000 /
0xFFC00000) nor gfx950's (0x7FC00000), so a kernel does not write it by accident.  Band width: every region has on each side at least
256 KiB and at least two rows of its own (`row_bytes`); two neighbours do not share a band, so damage is attributed to one region and
one side.  Regions start 256-byte aligned plus `align_off` bytes.  The comparison runs where the arena lives (torch.equal on slices
against a pristine copy); bytes travel to the host only to describe a failure.

What this sees: stray writes around the caller's buffers and writes to inputs.  Over-reads only when they change a result.  Buffers
the library allocates itself are outside the arena and are not covered."""
from __future__ import annotations

import numpy as np

PATTERN = 0x7FF8A5A5
MIN_BAND = 256 << 10
ALIGN = 256
_PAT_BYTES = np.array([PATTERN], "<u4").view(np.uint8)


def pattern_bytes(nbytes: int, phase: int = 0) -> np.ndarray:
    """`nbytes` of the band pattern as it lies at byte offset `phase` of the arena."""
    reps = -(-(nbytes + 4) // 4)
    return np.tile(_PAT_BYTES, reps)[phase % 4:phase % 4 + nbytes].copy()


class Region:
    """One caller buffer inside the arena.  `.addr` is its address (valid once the arena is laid out, which the first use does)."""

    def __init__(self, arena, name, kind, nbytes, align_off, row_bytes, data):
        self.arena, self.name, self.kind, self.nbytes = arena, name, kind, int(nbytes)
        self.align_off, self.row_bytes, self.data = int(align_off), int(row_bytes or 0), data
        self.band = max(MIN_BAND, 2 * self.row_bytes)
        self.start = None  # byte offset from the arena's aligned base

    @property
    def addr(self) -> int:
        self.arena._finalise()
        return self.arena.base + self.start

    def __int__(self):
        return self.addr

    __index__ = __int__


class RedzoneError(AssertionError):
    """`findings`: one dict per damaged place -- region, side ("before" / "after" / "input"), first, last (byte offsets relative to
    the region's edge: its end for "after", its start otherwise, so -1 is the byte right before it), changed (bytes), rows."""

    def __init__(self, msg, findings):
        super().__init__(msg)
        self.findings = findings


class Arena:
    def __init__(self, device="cuda", what=""):
        self.device, self.what, self.regions = device, what, []
        self.buf = self.pristine = None
        self.base = self.shift = self.total = 0

    # ---- requests ---------------------------------------------------------------------------------------------------------------
    def _add(self, name, kind, nbytes, align_off, row_bytes, data):
        if self.buf is not None:
            raise RuntimeError("the arena is laid out: ask for every region before the first address is used")
        if align_off < 0 or align_off >= ALIGN:
            raise ValueError("align_off is a byte count below 256")
        r = Region(self, name or f"{kind}{len(self.regions)}", kind, nbytes, align_off, row_bytes, data)
        self.regions.append(r)
        return r

    @staticmethod
    def _bytes(array):
        a = np.ascontiguousarray(array)
        return a.reshape(-1).view(np.uint8) if a.size else np.zeros(0, np.uint8)

    def input(self, array, align_off=0, row_bytes=None, name=None) -> Region:
        """A buffer the call only reads: uploaded, and compared with its snapshot by verify()."""
        b = self._bytes(array)
        return self._add(name, "input", b.size, align_off, row_bytes, b)

    def output(self, nbytes, align_off=0, prefill=None, row_bytes=None, name=None) -> Region:
        """A buffer the call writes: filled with the band pattern, or with `prefill` where the call accumulates into it."""
        data = None if prefill is None else self._bytes(prefill)
        if data is not None and data.size != nbytes:
            raise ValueError("prefill must be nbytes long")
        return self._add(name, "output", nbytes, align_off, row_bytes, data)

    def inout(self, array, align_off=0, row_bytes=None, name=None) -> Region:
        """A buffer the call transforms in place: uploaded, not compared."""
        b = self._bytes(array)
        return self._add(name, "inout", b.size, align_off, row_bytes, b)

    # ---- layout -----------------------------------------------------------------------------------------------------------------
    def layout(self):
        """Assign the regions' offsets (no allocation): returns the arena's size in bytes."""
        cur = 0
        for r in self.regions:
            r.start = -(-(cur + r.band) // ALIGN) * ALIGN + r.align_off
            cur = r.start + r.nbytes + r.band
            r.lo, r.hi = r.start - r.band, cur  # [lo, start) is its band before, [end, hi) its band after
        self.total = -(-max(cur, 4) // 4) * 4
        return self.total

    def _finalise(self):
        if self.buf is not None:
            return
        total = self.layout()
        if self.device == "host":
            store = np.empty(total + ALIGN, np.uint8)
            ptr = store.ctypes.data
        else:
            import torch

            store = torch.empty(total + ALIGN, dtype=torch.uint8, device=self.device)
            ptr = store.data_ptr()
        if ptr % 4:
            raise RuntimeError("allocation not 4-byte aligned")
        self.shift = (-ptr) % ALIGN
        self.base = ptr + self.shift
        img = pattern_bytes(total)
        for r in self.regions:
            if r.data is not None:
                img[r.start:r.start + r.nbytes] = r.data
            r.data = None
        if self.device == "host":
            self._store = store
            self.buf = store[self.shift:self.shift + total]
            self.buf[:] = img
            self.pristine = img
        else:
            import torch

            self._store = store
            self.buf = store[self.shift:self.shift + total]
            self.buf.copy_(torch.from_numpy(img))
            self.pristine = self.buf.clone()
            if self.buf.is_cuda:
                torch.cuda.synchronize()

    # ---- access -----------------------------------------------------------------------------------------------------------------
    def _region(self, r) -> Region:
        if isinstance(r, Region):
            return r
        self._finalise()
        for q in self.regions:
            if q.start + self.base == int(r):
                return q
        raise KeyError(f"no region at address {int(r):#x}")

    def _host(self, lo, hi, pristine=False) -> np.ndarray:
        src = self.pristine if pristine else self.buf
        if self.device == "host":
            return np.array(src[lo:hi], copy=True)
        return src[lo:hi].cpu().numpy()

    def _same(self, lo, hi) -> bool:
        if hi <= lo:
            return True
        if self.device == "host":
            return bool(np.array_equal(self.buf[lo:hi], self.pristine[lo:hi]))
        import torch

        return bool(torch.equal(self.buf[lo:hi], self.pristine[lo:hi]))

    def sync(self):
        if self.device not in ("host", "cpu"):
            import torch

            torch.cuda.synchronize()

    def read(self, region, dtype, shape) -> np.ndarray:
        """A numpy copy of a region's bytes as `dtype` in `shape` (the whole region)."""
        self._finalise()
        r = self._region(region)
        self.sync()
        return self._host(r.start, r.start + r.nbytes).view(dtype).reshape(shape)

    def restore(self, region):
        """Put a region's first bytes back (an in-place or accumulating buffer before a second run of the call)."""
        self._finalise()
        r = self._region(region)
        self.sync()
        self.buf[r.start:r.start + r.nbytes] = self.pristine[r.start:r.start + r.nbytes]
        self.sync()

    def poke(self, offset, data):
        """Overwrite bytes at an arena offset (the helper's own tests plant damage with this)."""
        self._finalise()
        b = self._bytes(data)
        if self.device == "host":
            self.buf[offset:offset + b.size] = b
        else:
            import torch

            self.buf[offset:offset + b.size] = torch.from_numpy(b.copy()).to(self.buf.device)

    # ---- the check --------------------------------------------------------------------------------------------------------------
    def _describe(self, r, side, lo, hi, edge):
        now, was = self._host(lo, hi), self._host(lo, hi, pristine=True)
        bad = np.flatnonzero(now != was)
        first, last = int(bad[0]) + lo - edge, int(bad[-1]) + lo - edge
        span = last - first + 1
        f = {"region": r.name, "side": side, "first": first, "last": last, "changed": int(bad.size), "span": span,
             "rows": span / r.row_bytes if r.row_bytes else None}
        if side == "input":
            return f, f"input '{r.name}' was modified: {bad.size} bytes changed, first at byte {first}, last at byte {last} of {r.nbytes}"
        rows = f", a run of {span / r.row_bytes:g} rows of {r.row_bytes} bytes" if r.row_bytes else ""
        rel = "end" if side == "after" else "start"
        return f, (f"write {side} {r.kind} '{r.name}': {bad.size} bytes changed, first at byte {first:+d}, last at byte {last:+d} from the region's {rel} "
                   f"(span {span} bytes{rows})")

    def verify(self, what=None):
        """Every band still holds the pattern and every input its bytes, or RedzoneError with one line per damaged place."""
        self._finalise()
        self.sync()
        findings, lines = [], []
        for r in self.regions:
            end = r.start + r.nbytes
            checks = [("before", r.lo, r.start, r.start), ("after", end, r.hi, end)]
            if r.kind == "input":
                checks.append(("input", r.start, end, r.start))
            for side, lo, hi, edge in checks:
                if not self._same(lo, hi):
                    f, line = self._describe(r, side, lo, hi, edge)
                    findings.append(f)
                    lines.append(line)
        last = self.regions[-1].hi if self.regions else 0
        if not self._same(last, self.total):
            lines.append("write in the arena's tail")
            findings.append({"region": None, "side": "tail"})
        if findings:
            raise RedzoneError(f"{what or self.what}: guard bands violated\n  " + "\n  ".join(lines), findings)
