"""The drawn cases of the filter and lapped fuzz (tests/test_gpu_filter_fuzz.py): a generator and a classifier, pure
Python and numpy -- nothing here imports torch or the library, so the coverage of the draw is checked without a GPU
(tests/test_filter_cases_cpu.py).  The four context-free host helpers of the library (kofft_hip_resample_route, kofft_hip_sosfilt_route,
kofft_hip_sosfilt_scan_chunk, kofft_hip_convolve_block) are handed in by the caller as a `Helpers`; the oracles are imported where a
function needs them.

cases(seed, helpers) is deterministic from np.random.default_rng(33000 + seed): 10 cases, each ONE call of one family -- resample,
sosfilt, sosfilt_scan, convolve_bank, dct4 (kofft_hip_dct4_fast_f32), mdct or imdct -- with a route (the value of the family's setter;
sosfilt_scan has none), a form and a data kind.  The forms: host; dev; dev_off, every f32 pointer 4 bytes off a 16-byte boundary (complex
outputs 8); dev_unaligned (convolve_bank and the DCT-IV family), dev_off with the main input two more bytes off, so no longer 4-byte
aligned: the header sends it through the composed route; inplace, where the header allows it.  Family, route and form take turns over the valid cases
(COMBOS: 63 entries, every one at least twice in the 144 valid cases of the 16 seeds); context, geometry and data are drawn.  One
case per seed is a call the header refuses (REFUSALS, by turns), built as a valid case with one argument replaced: it carries the code.
One case per seed is preceded by kofft_hip_release_scratch and one valid case runs on a side stream.

Size caps (the smallest shapes at which the kernels change behaviour; nothing approaches a workload size): resample: rows * max(nx,
out_len) <= 2^20 and rows * out_len * terms <= 2^23 (the oracle adds one term at a time); sosfilt and sosfilt_scan: nx * sections <= 2^15
(sosfilt_ref loops over samples and sections in Python); convolve_bank: rows * filters * nb * block <= 2^20; dct4 / mdct / imdct: rows *
frames * N <= 2^20.

sosfilt_scan in pieces.  The states of a call are rows * C * D * 4 bytes, C = ceil(nx / chunk) and D = 2 min(sections, 8); with nx *
sections <= 2^15 and chunk >= 32 that is at most 8 KiB a row, so no call of 65 rows or fewer exceeds 1 MiB: the cases that go in pieces of
whole rows on the 1 MiB context take their rows from PIECES (129 .. 257 rows), outside the list of the other cases."""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from math import gcd
from pathlib import Path
from typing import Optional

import numpy as np

F = np.float32
SEEDS = 16
PER_SEED = 10
CHUNK_DEFAULT = 512 << 20        # kScratchChunkDefaultBytes (host_layout.h)
CHUNK_1MB = 1 << 20              # KOFFT_HIP_SCRATCH_CHUNK_MB=1
MAX_POINTS = 1 << 20
RESAMPLE_MAX_TERMS = 1 << 23
SOS_MAX_STEPS = 1 << 15

# the codes of include/kofft_hip.h
OK, EMPTY_INPUT, NON_POWER_OF_TWO, MISMATCHED_LENGTHS, INVALID_VALUE, UNSUPPORTED, NULL = 0, 1, 2, 3, 6, -2, -3

_HEADER = (Path(__file__).resolve().parent.parent / "include" / "kofft_hip.h").read_text()


def _define(name: str) -> int:
    return int(re.search(rf"#define KOFFT_HIP_{name} (\d+)", _HEADER).group(1))


T = _define("SOSFILT_TILE")
G = _define("SOSFILT_GROUP")
TILE = _define("RESAMPLE_TILE")

SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.2e-38, 3e38, -3e38, np.inf, -np.inf, np.nan], F)  # test_gpu_rowwise_fuzz.py

FAMILIES = ["resample", "sosfilt", "sosfilt_scan", "convolve_bank", "dct4", "mdct", "imdct"]
ROUTES = {"resample": [0, 1, 2], "sosfilt": [0, 1, 2], "sosfilt_scan": [1], "convolve_bank": [0, 1], "dct4": [0, 1], "mdct": [0, 1], "imdct": [0, 1]}
FORMS = {"resample": ["host", "dev", "dev_off"], "sosfilt": ["host", "dev", "dev_off", "inplace"],
         "sosfilt_scan": ["host", "dev", "dev_off", "inplace"], "convolve_bank": ["host", "dev", "dev_off", "dev_unaligned"],
         "dct4": ["host", "dev", "dev_off", "dev_unaligned", "inplace"], "mdct": ["host", "dev", "dev_off", "dev_unaligned"],
         "imdct": ["host", "dev", "dev_off", "dev_unaligned"]}
# (sosfilt_scan has one route: its four forms stand twice in the list, so that its edge classes get as many cases as the others')
_ALL = [(fam, r, form) for fam in FAMILIES for r in ROUTES[fam] for form in FORMS[fam]] + [("sosfilt_scan", 1, form) for form in FORMS["sosfilt_scan"]]
COMBOS = [_ALL[i] for i in np.random.default_rng(32999).permutation(len(_ALL))]  # (a fixed shuffle: every seed holds several families)
VALID_PER_SEED = PER_SEED - 1


def _side_stream_families():
    """The family whose case runs on a side stream, per seed: of the families among the seed's valid cases (their turns are fixed by
    COMBOS) the one that had the side stream least often in the seeds before."""
    served = {fam: 0 for fam in FAMILIES}
    out = []
    for seed in range(SEEDS):
        here = {COMBOS[(seed * VALID_PER_SEED + k) % len(COMBOS)][0] for k in range(VALID_PER_SEED)}
        fam = min((f for f in FAMILIES if f in here), key=lambda f: served[f])
        served[fam] += 1
        out.append(fam)
    return out


SIDE_STREAM_FAMILY = _side_stream_families()

RATES = [(1, 1), (1, 2), (1, 3), (2, 1), (3, 1), (3, 2), (2, 3), (4, 2), (7, 5), (160, 441), (441, 160)]  # test_gpu_resample.py
RESAMPLE_ROWS = [1, 2, 3, 255, 256, 257]
RESAMPLE_OUT = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
SOS_ROWS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257]
SCAN_ROWS = [1, 2, 3, 63, 64, 65]
SCAN_CHUNKS = [T, 2 * T, 3 * T, 1024]
PIECES = [(8, 4096, 129), (8, 4095, 130), (7, 4096, 200), (16, 2048, 257)]  # (sections, nx, rows) at chunk T: the states exceed 1 MiB
BANK_ROWS = [1, 2, 3, 17]
BANK_FILTERS = [1, 2, 5]
XPB = {5: 32, 6: 16, 7: 16, 8: 16, 9: 4, 10: 4, 11: 2, 12: 1}  # items per workgroup of the fused DCT-IV kernel, by log2 (N / 2)
FUSED_N = [64 << i for i in range(8)]
COMPOSED_N = [2, 6, 32, 240, 960, 16384]

# (family, what) of the refused call of seed s: REFUSALS[s % len]
REFUSALS = [("resample", "past_end"), ("sosfilt", "flag"), ("sosfilt_scan", "chunk_off_tile"), ("convolve_bank", "block<nh"), ("dct4", "odd"),
            ("mdct", "lead"), ("imdct", "window"), ("resample", "up0"), ("sosfilt_scan", "chunk0"), ("convolve_bank", "kind3"), ("mdct", "odd"),
            ("convolve_bank", "nonpow2"), ("sosfilt", "sections0"), ("convolve_bank", "flag"), ("mdct", "stride"), ("imdct", "odd")]


def is_pow2(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


class Helpers:
    """The library's context-free host helpers as plain functions of ints.  from_lib(lib): `lib` is the loaded ctypes library."""

    def __init__(self, resample_route, sosfilt_route, scan_chunk, convolve_block):
        self.resample_route, self.sosfilt_route, self.scan_chunk, self.convolve_block = resample_route, sosfilt_route, scan_chunk, convolve_block
        self._flip = {}

    @classmethod
    def from_lib(cls, lib):
        import ctypes as C

        def resample_route(nh, up, down):
            r = C.c_int(-1)
            assert lib.kofft_hip_resample_route(nh, up, down, C.byref(r)) == 0
            return r.value

        def sosfilt_route(rows):
            r = C.c_int(-1)
            assert lib.kofft_hip_sosfilt_route(rows, C.byref(r)) == 0
            return r.value

        def scan_chunk(rows, nx, sections):
            k = C.c_size_t(0)
            assert lib.kofft_hip_sosfilt_scan_chunk(rows, nx, sections, C.byref(k)) == 0
            return k.value

        def convolve_block(nx, nh):
            k = C.c_size_t(0)
            assert lib.kofft_hip_convolve_block(nx, nh, C.byref(k)) == 0
            return k.value

        return cls(resample_route, sosfilt_route, scan_chunk, convolve_block)

    def flip_nh(self, up: int, down: int) -> Optional[int]:
        """The largest nh at which a default context runs the tiled resampler (the header: the route is 1 up to some nh and 0 beyond),
        by bisection; None where nh = 1 already runs the plain kernel or nothing below 2^20 taps does."""
        key = (up, down)
        if key not in self._flip:
            lo, hi = 1, 1 << 20
            if self.resample_route(lo, up, down) != 1 or self.resample_route(hi, up, down) != 0:
                self._flip[key] = None
            else:
                while hi - lo > 1:
                    mid = (lo + hi) // 2
                    if self.resample_route(mid, up, down) == 1:
                        lo = mid
                    else:
                        hi = mid
                self._flip[key] = lo
        return self._flip[key]


@dataclass
class Case:
    """One call.  g: the family's geometry (sizes, flags, and the `*_kind` tags the draw leaves for the classifier)."""
    seed: int
    index: int
    family: str
    route: int
    form: str
    ctx: str                      # "default" or "chunk1"
    specials: bool
    data_seed: int
    g: dict
    refuse: Optional[dict] = None  # {"what", "code", "args": {name: value}}: the arguments replaced in the call
    release_before: bool = False  # kofft_hip_release_scratch right before this case
    side_stream: bool = False
    tags: set = field(default_factory=set)

    @property
    def x_off2(self) -> bool:
        """the main input is not 4-byte aligned: the composed route"""
        return self.form == "dev_unaligned"

    @property
    def cap(self) -> int:
        return CHUNK_1MB if self.ctx == "chunk1" else CHUNK_DEFAULT

    def describe(self) -> str:
        geo = " ".join(f"{k}={v}" for k, v in self.g.items())
        extra = (" x_off2" if self.x_off2 else "") + (f" refuse={self.refuse['what']}->{self.refuse['code']}" if self.refuse else "")
        return (f"seed={self.seed} case={self.index} family={self.family} route={self.route} form={self.form} ctx={self.ctx} "
                f"specials={self.specials} {geo}{extra}")


# ---- small arithmetic, restated from the host sources ---------------------------------------------------------------------------------
def chunk_rows(cap_bytes: int, row_bytes: int, count: int) -> int:
    """scratch_chunk_rows (host_layout.h): cap / row bytes, at least 1, at most count; count 0: 0."""
    if count == 0:
        return 0
    chunk = cap_bytes // row_bytes if row_bytes else count
    return min(max(chunk, 1), count)


def resample_full_up(g) -> int:
    return (g["nx"] - 1) * g["up"] + g["nh"]


def resample_terms(nh: int, up: int) -> int:
    return (nh - 1) // up + 1


def scan_chunks(nx: int, chunk: int) -> int:
    return (nx - 1) // chunk + 1


def scan_piece_rows(case: Case) -> int:
    """k_sosfilt_f32.hip, kofft_hip_dev_sosfilt_scan_f32: the rows per piece, C * Dmax * 4 bytes of states a row (C == 1: no states)."""
    g = case.g
    C = scan_chunks(g["nx"], g["chunk"])
    dmax = 2 * min(g["sections"], G)
    return chunk_rows(case.cap, C * dmax * 4 if C > 1 else 0, g["rows"])


def bank_shape(g):
    """(hop, full, nb, b0, nbw): the blocks of a row and those the window touches (convolve_shape, k_convolve_f32.hip)."""
    hop = g["block"] - g["nh"] + 1
    full = g["nx"] + g["nh"] - 1
    b0 = g["out_first"] // hop
    nbw = (g["out_first"] + g["out_len"] - 1) // hop - b0 + 1
    return hop, full, ceil_div(full, hop), b0, nbw


def bank_fused(case: Case) -> bool:
    """conv_fused_ok: the switch on, blocks 32 .. 4096, x 4-byte aligned."""
    return bool(case.route) and 32 <= case.g["block"] <= 4096 and not case.x_off2


def dct_fused(case: Case) -> bool:
    """dct4_fused_ok: the switch on, N a power of two 64 .. 8192, the inputs 4-byte aligned."""
    n = case.g["n"]
    return bool(case.route) and is_pow2(n) and 64 <= n <= 8192 and not case.x_off2


def dct_items(case: Case) -> int:
    g = case.g
    return g["rows"] * g.get("frames", 1)


def mdct_frames_past(g) -> int:
    """the frames of a row that hold no sample: f N - lead >= nx"""
    return sum(1 for f in range(g["frames"]) if f * g["n"] - g["lead"] >= g["nx"])


# ---- the classifier ---------------------------------------------------------------------------------------------------------------------
def classify(case: Case, helpers: Helpers) -> set:
    fam, g = case.family, case.g
    c = {f"{fam}:route{case.route}:{case.form}", f"ctx:{case.ctx}", f"family:{fam}"}
    if case.refuse:
        return c | {"refusal", f"refusal:{fam}"}
    if case.specials:
        c.add("specials")
    if case.release_before:
        c.add("release_before")
    if case.side_stream:
        c.add("side_stream")
    if fam == "resample":
        up, down, nh, out_len = g["up"], g["down"], g["nh"], g["out_len"]
        flip = helpers.flip_nh(up, down)
        if flip is not None and flip - 1 <= nh <= flip + 2:  # (flip: the last nh on the tiled kernel, flip + 1: the first on the plain one)
            c.add("resample:route_flip")
        c.add("resample:kernel_tiled" if (case.route == 2 or (case.route == 1 and helpers.resample_route(nh, up, down) == 1)) else "resample:kernel_plain")
        if nh in (1, up - 1, up, up + 1):
            c.add("resample:nh_at_up")
        if nh == 1:
            c.add("resample:one_tap")
        if gcd(up, down) > 1:
            c.add("resample:not_coprime")
        if out_len in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
            c.add("resample:tile_edge")
        if out_len == 1:
            c.add("resample:one_output")
        if g["rows"] >= 255:
            c.add("resample:rows_at_256")
        c.add(f"resample:t0_{g['t0_kind']}")
        if g["out_kind"] == "full":
            c.add("resample:full_length")
    elif fam in ("sosfilt", "sosfilt_scan"):
        rows, nx, sections = g["rows"], g["nx"], g["sections"]
        if sections in (G - 1, G, G + 1, 2 * G, 2 * G + 1):
            c.add(f"{fam}:group_edge")
        if sections > G:
            c.add(f"{fam}:many_passes")
        c.add(f"{fam}:{'zi' if g['zi'] else 'no_zi'}")
        c.add(f"{fam}:{'zf' if g['zf'] else 'no_zf'}")
        c.add(f"{fam}:{'reverse' if g['reverse'] else 'forward'}")
        if fam == "sosfilt":
            if rows in (15, 16, 17):
                c.add("sosfilt:route_edge_16_rows")
            if rows in (63, 64, 65, 127, 128, 129):
                c.add("sosfilt:wave_edge_64_rows")
            if nx in (T - 1, T, T + 1, 2 * T + 1):
                c.add("sosfilt:tile_edge")
            if nx <= 2:
                c.add("sosfilt:tiny_row")
            tiled = case.route == 2 or (case.route == 1 and helpers.sosfilt_route(rows) == 1)
            c.add("sosfilt:kernel_tiled" if tiled else "sosfilt:kernel_plain")
        else:
            C = scan_chunks(nx, g["chunk"])
            c.add(f"sosfilt_scan:chunk{g['chunk']}")
            if C in (63, 64, 65):
                c.add("sosfilt_scan:64_chunk_edge")
            if nx % g["chunk"] in (0, 1, g["chunk"] - 1):
                c.add("sosfilt_scan:nx_at_chunk_multiple")
            if C == 1:
                c.add("sosfilt_scan:one_chunk")
            if scan_piece_rows(case) < rows:
                c.add("sosfilt_scan:pieces_of_rows")
            if rows in (63, 64, 65):
                c.add("sosfilt_scan:rows_at_64")
    elif fam == "convolve_bank":
        block = g["block"]
        hop, full, nb, b0, nbw = bank_shape(g)
        c.add("bank:fused" if bank_fused(case) else "bank:small" if block < 32 else "bank:composed")
        if block in (16, 8192):
            c.add("bank:fused_range_neighbour")
        if block in (32, 4096):
            c.add("bank:fused_range_end")
        if case.x_off2 and case.route and 32 <= block <= 4096:
            c.add("bank:off_alignment_composed")
        c.add("bank:complex_taps" if g["complex_taps"] else "bank:real_taps")
        if g["correlate"]:
            c.add("bank:correlate")
        c.add(f"bank:out_{g['kind']}")
        c.add(f"bank:window_{g['window']}")
        c.add(f"bank:filters{g['filters']}")
        if hop == 1:
            c.add("bank:hop1")
        c.add("bank:one_block" if nb == 1 else "bank:many_blocks")
        if not bank_fused(case) and chunk_rows(case.cap, 2 * block * 8, g["rows"] * nbw) < g["rows"] * nbw:
            c.add("bank:chunk_seam")
    else:
        n = g["n"]
        fused = dct_fused(case)
        c.add("dct:fused" if fused else "dct:composed")
        c.add(f"{fam}:{'fused' if fused else 'composed'}")
        if n in COMPOSED_N:
            c.add("dct:composed_only_n")
        if not is_pow2(n // 2):
            c.add("dct:bluestein")
        if case.x_off2 and case.route and is_pow2(n) and 64 <= n <= 8192:
            c.add("dct:off_alignment_composed")
        items = dct_items(case)
        if n in FUSED_N:
            xpb = XPB[(n // 2).bit_length() - 1]
            if xpb > 1 and items > xpb and items % xpb in (0, 1, xpb - 1):
                c.add("dct:items_at_workgroup_multiple")
            if items > xpb:
                c.add("dct:many_workgroups")
        if not fused and chunk_rows(case.cap, (n // 2) * 8, items) < items:
            c.add("dct:chunk_seam")
        if fam == "mdct":
            c.add("mdct:lead_0" if g["lead"] == 0 else "mdct:lead_n" if g["lead"] == n else "mdct:lead_other")
            past = mdct_frames_past(g)
            if past:
                c.add("mdct:frames_past_the_end")
            if g["rows"] > 1 and g["row_stride"] > g["nx"]:
                c.add("mdct:stride_gap")
            if g["rows"] > 1:
                c.add("mdct:rows>1")
        if fam == "imdct":
            c.add(f"imdct:window_{g['window']}")
            c.add("imdct:scale_2/n" if g["scale_kind"] == "2/n" else "imdct:scale_other")
            if g["frames"] == 1:
                c.add("imdct:one_frame")
            if chunk_rows(case.cap, n * 4, items) < items:
                c.add("imdct:chunk_seam")
    return c


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _sections(rng, most: int) -> int:
    s = int(_pick(rng, [1, G - 1, G, G + 1, 2 * G, 2 * G + 1])) if rng.random() < 0.75 else int(rng.integers(1, 2 * G + 2))
    return max(1, min(s, most))


def _resample(rng, helpers, turn):
    up, down = RATES[int(rng.integers(0, len(RATES)))] if turn % 2 == 0 else (int(rng.integers(1, 17)), int(rng.integers(1, 17)))
    if turn % 4 == 1 and gcd(up, down) == 1:
        up, down = 2 * up, 2 * down  # (a pair that is not coprime, by turns: no gcd reduction happens)
    flip = helpers.flip_nh(up, down)
    kinds = ["one", "up-1", "up", "up+1", "random", "random", "flip-1", "flip", "flip+1"]
    kind = kinds[turn % len(kinds)] if rng.random() < 0.6 else _pick(rng, kinds)
    if kind.startswith("flip") and flip is None:
        kind = "random"
    nh = {"one": 1, "up-1": up - 1, "up": up, "up+1": up + 1, "random": int(rng.integers(1, 4101)),
          "flip-1": (flip or 0) - 1, "flip": flip or 0, "flip+1": (flip or 0) + 1}[kind]
    nh = max(1, nh)
    terms = resample_terms(nh, up)
    rows = int(_pick(rng, RESAMPLE_ROWS))
    out_kind = _pick(rng, ["one", "full", "tile", "tile", "random"])
    t0_kind = _pick(rng, ["zero", "centre", "random"])
    if out_kind == "full":
        nx = int(rng.integers(1, 601))
        full_up = (nx - 1) * up + nh
        t0 = {"zero": 0, "centre": (nh - 1) // 2, "random": int(rng.integers(0, full_up))}[t0_kind]
        out_len = ceil_div(full_up - t0, down)
        if out_len * terms > RESAMPLE_MAX_TERMS:  # (many taps: the whole result costs the oracle too much)
            out_kind = "random"
    if out_kind != "full":
        out_len = {"one": 1, "tile": int(_pick(rng, RESAMPLE_OUT[1:])), "random": int(rng.integers(2, 3001))}[out_kind]
        out_len = max(1, min(out_len, RESAMPLE_MAX_TERMS // terms))
        t0 = {"zero": 0, "centre": (nh - 1) // 2, "random": int(rng.integers(0, nh + 4 * up))}[t0_kind]
        need = t0 + (out_len - 1) * down + 1 - nh  # (nx - 1) * up must exceed need - 1
        nx = max(1, ceil_div(max(need, 0), up) + 1) + int(rng.integers(0, 4))
    most = min(MAX_POINTS // max(nx, out_len), RESAMPLE_MAX_TERMS // (out_len * terms))
    if rows > most:
        rows = max([r for r in RESAMPLE_ROWS if r <= most] or [1])
    g = dict(rows=rows, nx=nx, nh=nh, up=up, down=down, t0=t0, out_len=out_len, nh_kind=kind, t0_kind=t0_kind, out_kind=out_kind)
    assert t0 + (out_len - 1) * down < resample_full_up(g), g
    return g


def _sosfilt(rng, helpers, turn):
    rows = int(SOS_ROWS[turn % len(SOS_ROWS)]) if rng.random() < 0.5 else int(_pick(rng, SOS_ROWS))
    nx = int(_pick(rng, [1, 2, T - 1, T, T + 1, 2 * T + 1, int(rng.integers(1, 4001)), int(rng.integers(1, 4001))]))
    return dict(rows=rows, nx=nx, sections=_sections(rng, SOS_MAX_STEPS // nx), zi=bool(rng.random() < 0.6), zf=bool(rng.random() < 0.6),
                reverse=bool(rng.random() < 0.5))


def _scan(rng, helpers, turn, ctx):
    kind = ["c64", "pieces", "few", "c64"][turn % 4]
    if kind == "pieces" and ctx != "chunk1":
        kind = "c64"
    if kind == "pieces":
        sections, nx, rows = PIECES[(turn // 4) % len(PIECES)]
        chunk = T
    else:
        rows = int(_pick(rng, SCAN_ROWS))
        if kind == "c64":
            chunk = int(SCAN_CHUNKS[(turn // 2) % 3])
            nx = int(_pick(rng, [63, 64, 65])) * chunk + int(rng.integers(-1, 2))
        else:
            chunk = int([1024, T, helpers.scan_chunk(rows, 4 * 1024, 1), 2 * T, 1024, 3 * T][(turn // 4) % 6])  # (the rule's own choice: 1024 here)
            m = 1 if (turn // 4) % 2 == 0 else int(rng.integers(2, 5))  # (one chunk, C == 1, by turns: sosfilt's own bytes)
            nx = max(1, m * chunk + (int(rng.integers(-1, 1)) if m == 1 else int(rng.integers(-1, 2))))
            while nx > SOS_MAX_STEPS:
                nx -= chunk
        sections = _sections(rng, SOS_MAX_STEPS // nx)
    return dict(rows=rows, nx=nx, sections=sections, chunk=chunk, zi=bool(rng.random() < 0.6), zf=bool(rng.random() < 0.6),
                reverse=bool(rng.random() < 0.5), scan_kind=kind)


BANK_BLOCKS = [16, 8192, 32, 4096, 2, 64, 1024, 8, 256, 4, 512, 2048, 128]  # by turns: the fused range's ends and neighbours first


def _bank(rng, helpers, turn, in_fused_range=False, fill=False):
    block = int(BANK_BLOCKS[turn % len(BANK_BLOCKS)]) if rng.random() < 0.6 else 1 << int(rng.integers(1, 14))
    if in_fused_range and not 32 <= block <= 4096:
        block = int(_pick(rng, [32, 64, 256, 1024, 4096]))
    taps = [1, 2, block // 2, block - 1, block]
    nh = max(1, int(taps[(turn // 2) % 5] if rng.random() < 0.6 else _pick(rng, taps)))
    rows, filters = int(_pick(rng, BANK_ROWS)), int(_pick(rng, BANK_FILTERS))
    if fill:  # the composed route on the 1 MiB context: 17 long rows, so that its 16 * block bytes per (row, block) fill more than one chunk
        rows, filters = 17, min(filters, 2)
    # the cap on rows * filters * nb * block: even nx == 1 takes ceil(nh / hop) blocks, so a long filter in a large block loses rows
    # and filters first, then taps
    most_blocks = MAX_POINTS // (rows * filters * block)
    if nh > most_blocks * (block + 1) // (1 + most_blocks):
        rows, filters = 1, min(filters, 2)
        most_blocks = MAX_POINTS // (filters * block)
        nh = max(1, min(nh, most_blocks * (block + 1) // (1 + most_blocks)))
    hop = block - nh + 1
    nx = max(1, int(_pick(rng, [1, nh - 1, hop - 1, hop, hop + 1, 3 * hop + 7, int(rng.integers(1, 5001)), int(rng.integers(1, 5001))])))
    if fill:
        nx = 5000
    nx = max(1, min(nx, most_blocks * hop - nh + 1))
    full = nx + nh - 1
    window = ["full", "same", "valid", "inside"][turn % 4]
    if window == "valid" and nx < nh:
        nx = min(nh + int(rng.integers(0, 8)), max(1, most_blocks * hop - nh + 1))
        full = nx + nh - 1
        if nx < nh:
            window = "full"
    if window == "full":
        first, count = 0, full
    elif window == "same":
        first, count = (nh - 1) // 2, nx
    elif window == "valid":
        first, count = nh - 1, nx - nh + 1
    else:
        first = int(rng.integers(0, full))
        count = int(rng.integers(1, full - first + 1))
    g = dict(rows=rows, nx=nx, nh=nh, filters=filters, block=block, complex_taps=bool(rng.random() < 0.5), correlate=bool(rng.random() < 0.5),
             kind=["real", "complex", "magnitude"][(turn // 4) % 3] if rng.random() < 0.7 else _pick(rng, ["real", "complex", "magnitude"]),
             window=window, out_first=first, out_len=count)
    assert rows * filters * ceil_div(full, hop) * block <= MAX_POINTS, g
    return g


def _dct_n(rng, route, turn, in_fused_range=False):
    if in_fused_range:
        return int(_pick(rng, FUSED_N))
    if route:
        return int(_pick(rng, FUSED_N)) if turn % 4 != 3 else int(_pick(rng, COMPOSED_N))
    return int(_pick(rng, FUSED_N)) if turn % 2 else int(COMPOSED_N[(turn // 2) % len(COMPOSED_N)])


def _items(rng, n, fill=False):
    """items of a DCT-IV call: within one of a multiple of the fused kernel's items per workgroup, inside the cap; fill: as many as the
    cap allows, so that the composed route's N / 2 complex points an item and the IMDCT's N floats exceed 1 MiB"""
    most = max(1, MAX_POINTS // n)
    xpb = XPB.get((n // 2).bit_length() - 1, 4) if is_pow2(n) else 4
    items = int(rng.integers(1, 4)) * xpb + int(rng.integers(-1, 2))
    if fill and n >= 32:
        items = most - int(rng.integers(0, 3))
    return max(1, min(items, most))


def _dct4(rng, route, turn, in_fused_range=False, fill=False):
    n = _dct_n(rng, route, turn, in_fused_range)
    return dict(n=n, rows=_items(rng, n, fill))


def _mdct(rng, route, turn, in_fused_range=False, fill=False):
    n = _dct_n(rng, route, turn, in_fused_range)
    items = _items(rng, n, fill)
    rows = int(_pick(rng, [1, 1, 2, 3, 5]))
    rows = min(rows, items)
    lead = int([0, n, int(rng.integers(0, 2 * n))][turn % 3]) if rng.random() < 0.7 else int(_pick(rng, [0, n, int(rng.integers(0, 2 * n))]))
    past = int(_pick(rng, [0, 0, 1, 2]))
    first_cover = max(1, ceil_div(lead + 1, n))  # the least `covered` with covered * n - lead >= 1
    frames = max(items // rows, 1)
    covered = max(frames - past, first_cover)
    frames = covered + past
    while rows > 1 and rows * frames * n > MAX_POINTS:
        rows -= 1
    if rows * frames * n > MAX_POINTS:
        frames = max(first_cover, MAX_POINTS // (rows * n))
        covered, past = frames, 0
    hi = covered * n - lead                      # frame `covered` is the first that holds no sample: nx <= hi
    lo = max(1, (covered - 1) * n - lead + 1)    # ... and frame covered - 1 holds one: nx > (covered - 1) * n - lead
    nx = int(rng.integers(lo, hi + 1))
    stride = nx + int([0, 1, int(rng.integers(2, 65))][int(rng.integers(0, 3))])
    g = dict(n=n, rows=rows, nx=nx, row_stride=stride, lead=lead, frames=frames, window_kind=_pick(rng, ["sine", "random"]))
    assert rows * frames * n <= MAX_POINTS, g
    return g


def _imdct(rng, route, turn, in_fused_range=False, fill=False):
    n = _dct_n(rng, route, turn, in_fused_range)
    items = _items(rng, n, fill)
    rows = min(int(_pick(rng, [1, 1, 2, 3, 5])), items)
    frames = max(items // rows, 1)
    full = (frames + 1) * n
    window = ["whole", "from_n", "random"][turn % 3]
    if window == "whole":
        first, count = 0, full
    elif window == "from_n":
        first, count = n, int(rng.integers(1, full - n + 1))
    else:
        first = int(rng.integers(0, full))
        count = int(rng.integers(1, full - first + 1))
    scale_kind = "2/n" if rng.random() < 0.5 else "other"
    return dict(n=n, rows=rows, frames=frames, out_first=first, out_len=count, window=window, scale_kind=scale_kind,
                scale=float(F(2.0 / n)) if scale_kind == "2/n" else float(F(rng.uniform(0.05, 1.5))))


def _geometry(rng, helpers, fam, route, turn, ctx, in_fused_range=False):
    fill = ctx == "chunk1" and turn % 2 == 0
    if fam == "resample":
        return _resample(rng, helpers, turn)
    if fam == "sosfilt":
        return _sosfilt(rng, helpers, turn)
    if fam == "sosfilt_scan":
        return _scan(rng, helpers, turn, ctx)
    if fam == "convolve_bank":
        return _bank(rng, helpers, turn, in_fused_range, fill=fill and not route)
    return {"dct4": _dct4, "mdct": _mdct, "imdct": _imdct}[fam](rng, route, turn, in_fused_range, fill)


def _refusal(case: Case, what: str) -> dict:
    """The arguments that turn the valid call into one the header refuses, and the code it names for them."""
    g = case.g
    if what == "past_end":   # t0 + (out_len - 1) * down >= full_up
        return dict(what=what, code=MISMATCHED_LENGTHS, args=dict(out_len=ceil_div(resample_full_up(g) - g["t0"], g["down"]) + 1))
    if what == "up0":
        return dict(what=what, code=INVALID_VALUE, args=dict(up=0))
    if what == "flag":       # an unknown flag bit
        return dict(what=what, code=INVALID_VALUE, args=dict(flags=16 if case.family == "convolve_bank" else 2))
    if what == "sections0":
        return dict(what=what, code=EMPTY_INPUT, args=dict(sections=0))
    if what == "chunk_off_tile":
        return dict(what=what, code=INVALID_VALUE, args=dict(chunk=g["chunk"] + 1))
    if what == "chunk0":
        return dict(what=what, code=INVALID_VALUE, args=dict(chunk=0))
    if what == "block<nh":
        return dict(what=what, code=MISMATCHED_LENGTHS, args=dict(block=1 << ((g["nh"] - 1).bit_length() - 1)))  # the power of two below nh >= 2
    if what == "kind3":
        return dict(what=what, code=INVALID_VALUE, args=dict(flags=12))
    if what == "nonpow2":
        return dict(what=what, code=NON_POWER_OF_TWO, args=dict(block=3 * g["block"]))
    if what == "odd":
        return dict(what=what, code=INVALID_VALUE, args=dict(n=g["n"] + 1))
    if what == "lead":
        return dict(what=what, code=INVALID_VALUE, args=dict(lead=2 * g["n"]))
    if what == "stride":     # rows > 1 and row_stride < nx
        return dict(what=what, code=INVALID_VALUE, args=dict(rows=max(2, g["rows"]), row_stride=g["nx"] - 1))
    if what == "window":     # out_first + out_len > full
        return dict(what=what, code=MISMATCHED_LENGTHS, args=dict(out_first=(g["frames"] + 1) * g["n"] - g["out_len"] + 1))
    raise KeyError(what)


def _draw(rng, helpers, seed, fam, route, form, turn) -> Case:
    ctx = "chunk1" if rng.random() < 0.5 else "default"
    if fam == "sosfilt_scan" and turn % 4 == 1:
        ctx = "chunk1"  # (the pieces of whole rows need the 1 MiB context)
    # (off 4-byte alignment with the fused route on: a size the fused kernel would take, so that the alignment alone decides)
    g = _geometry(rng, helpers, fam, route, turn, ctx, in_fused_range=form == "dev_unaligned" and bool(route))
    return Case(seed=seed, index=-1, family=fam, route=route, form=form, ctx=ctx, specials=bool(rng.random() < 0.25), data_seed=int(rng.integers(0, 1 << 31)),
                g=g)


def cases(seed: int, helpers: Helpers) -> list:
    rng = np.random.default_rng(33000 + seed)
    out = []
    for k in range(VALID_PER_SEED):
        v = seed * VALID_PER_SEED + k
        fam, route, form = COMBOS[v % len(COMBOS)]
        turn = sum(1 for u in range(v) if COMBOS[u % len(COMBOS)][0] == fam)  # the turn of a family: how many of its valid cases came before
        out.append(_draw(rng, helpers, seed, fam, route, form, turn))
    fam, what = REFUSALS[seed % len(REFUSALS)]
    route, form = int(_pick(rng, ROUTES[fam])), _pick(rng, FORMS[fam])
    if form in ("inplace", "dev_unaligned"):
        form = "dev"
    bad = _draw(rng, helpers, seed, fam, route, form, seed)
    bad.specials = False
    if what == "block<nh" and bad.g["nh"] < 2:
        bad.g["nh"] = 2
        bad.g["block"] = max(bad.g["block"], 2)
    bad.refuse = _refusal(bad, what)
    out.insert(int(rng.integers(0, len(out) + 1)), bad)
    order = rng.permutation(len(out))
    out = [out[i] for i in order]
    for i, c in enumerate(out):
        c.index = i
    out[int(rng.integers(1, len(out)))].release_before = True
    next(c for c in out if not c.refuse and c.family == SIDE_STREAM_FAMILY[seed % SEEDS]).side_stream = True
    return out


# ---- the call's scalar arguments --------------------------------------------------------------------------------------------------------
def call_args(case: Case) -> dict:
    """The scalar arguments of the C call by name, the refused case's replacements applied."""
    g = case.g
    fam = case.family
    if fam == "resample":
        a = {k: g[k] for k in ("rows", "nx", "nh", "up", "down", "t0", "out_len")}
    elif fam in ("sosfilt", "sosfilt_scan"):
        a = dict(rows=g["rows"], nx=g["nx"], sections=g["sections"], flags=1 if g["reverse"] else 0)
        if fam == "sosfilt_scan":
            a["chunk"] = g["chunk"]
    elif fam == "convolve_bank":
        flags = (1 if g["correlate"] else 0) | (2 if g["complex_taps"] else 0) | ({"real": 0, "complex": 1, "magnitude": 2}[g["kind"]] << 2)
        a = dict(rows=g["rows"], nx=g["nx"], filters=g["filters"], nh=g["nh"], block=g["block"], flags=flags, out_first=g["out_first"],
                 out_len=g["out_len"])
    elif fam == "dct4":
        a = dict(n=g["n"], batch=g["rows"])
    elif fam == "mdct":
        a = {k: g[k] for k in ("rows", "nx", "row_stride", "n", "lead", "frames")}
    else:
        a = {k: g[k] for k in ("rows", "frames", "n", "scale", "out_first", "out_len")}
    if case.refuse:
        a.update(case.refuse["args"])
    return a


def invoke(fn, ctx, case: Case, p: dict) -> int:
    """Call the family's C entry `fn` (host or device form) with the pointers p (name -> address or None)."""
    import ctypes as C

    a = call_args(case)
    fam = case.family
    if fam == "resample":
        return fn(ctx, p["x"], a["rows"], a["nx"], p["h"], a["nh"], a["up"], a["down"], a["t0"], p["out"], a["out_len"])
    if fam == "sosfilt":
        return fn(ctx, p["x"], a["rows"], a["nx"], p["sos"], a["sections"], p.get("zi"), p.get("zf"), a["flags"], p["out"])
    if fam == "sosfilt_scan":
        return fn(ctx, p["x"], a["rows"], a["nx"], p["sos"], a["sections"], p.get("zi"), p.get("zf"), a["chunk"], a["flags"], p["out"])
    if fam == "convolve_bank":
        return fn(ctx, p["x"], a["rows"], a["nx"], p["h"], a["filters"], a["nh"], a["block"], a["flags"], p["out"], a["out_first"], a["out_len"])
    if fam == "dct4":
        return fn(ctx, p["x"], p["out"], a["n"], a["batch"])
    if fam == "mdct":
        return fn(ctx, p["x"], a["rows"], a["nx"], a["row_stride"], p["window"], a["n"], a["lead"], p["out"], a["frames"])
    return fn(ctx, p["x"], a["rows"], a["frames"], p["window"], a["n"], C.c_float(a["scale"]), p["out"], a["out_first"], a["out_len"])


ENTRY = {"resample": "resample_f32", "sosfilt": "sosfilt_f32", "sosfilt_scan": "sosfilt_scan_f32", "convolve_bank": "convolve_bank_f32",
         "dct4": "dct4_fast_f32", "mdct": "mdct_f32", "imdct": "imdct_f32"}


def header_violations(case: Case) -> list:
    """Every precondition of the family's header block that the call's arguments break (empty: a valid call)."""
    a = call_args(case)
    fam = case.family
    bad = []
    if fam == "resample":
        if a["nx"] == 0 or a["nh"] == 0:
            bad.append("empty")
        if a["up"] == 0 or a["down"] == 0:
            bad.append("up or down == 0")
        elif a["t0"] + (a["out_len"] - 1) * a["down"] >= (a["nx"] - 1) * a["up"] + a["nh"]:
            bad.append("an output wholly past the result")
    elif fam in ("sosfilt", "sosfilt_scan"):
        if a["sections"] == 0:
            bad.append("no sections")
        if a["flags"] & ~1:
            bad.append("an unknown flag bit")
        if fam == "sosfilt_scan" and (a["chunk"] == 0 or a["chunk"] % T):
            bad.append("chunk 0 or no multiple of the tile")
    elif fam == "convolve_bank":
        if not is_pow2(a["block"]):
            bad.append("block not a power of two")
        if a["block"] < a["nh"]:
            bad.append("block < nh")
        if a["out_first"] + a["out_len"] > a["nx"] + a["nh"] - 1:
            bad.append("window past the full result")
        if a["flags"] >> 4 or (a["flags"] >> 2) & 3 == 3:
            bad.append("flags")
        if a["block"] > 65536:
            bad.append("block > 65536")
    else:
        if a["n"] == 0 or a["n"] % 2:
            bad.append("N odd or 0")
        if fam == "mdct":
            if a["nx"] == 0:
                bad.append("nx == 0")
            if a["lead"] >= 2 * a["n"]:
                bad.append("lead >= 2N")
            if a["rows"] > 1 and a["row_stride"] < a["nx"]:
                bad.append("row_stride < nx")
        if fam == "imdct" and a["out_first"] + a["out_len"] > (a["frames"] + 1) * a["n"]:
            bad.append("window past the full result")
    return bad


def within_caps(case: Case) -> bool:
    g, fam = case.g, case.family
    if fam == "resample":
        return (g["rows"] * max(g["nx"], g["out_len"]) <= MAX_POINTS and
                g["rows"] * g["out_len"] * resample_terms(g["nh"], g["up"]) <= RESAMPLE_MAX_TERMS)
    if fam in ("sosfilt", "sosfilt_scan"):
        return g["nx"] * g["sections"] <= SOS_MAX_STEPS and 1 <= g["sections"] <= 2 * G + 1
    if fam == "convolve_bank":
        hop, full, nb, _, _ = bank_shape(g)
        return g["rows"] * g["filters"] * nb * g["block"] <= MAX_POINTS and 2 <= g["block"] <= 8192
    return dct_items(case) * g["n"] <= MAX_POINTS


# ---- the inputs of a case ---------------------------------------------------------------------------------------------------------------
def _data(rng, shape, specials):
    """uniform [-1, 1); with `specials` a few rows get special values (the three row kinds of test_gpu_rowwise_fuzz.py)"""
    x = rng.uniform(-1, 1, shape).astype(F)
    if specials and x.size:
        b, n = shape
        for r in rng.choice(b, size=min(b, 1 + int(rng.integers(0, 4))), replace=False):
            kind = int(rng.integers(0, 3))
            if kind == 0:    # a whole row of one special value
                x[r] = rng.choice(SPECIALS)
            elif kind == 1:  # a few specials in a uniform row
                pos = rng.choice(n, size=min(n, 1 + int(rng.integers(0, 3))), replace=False)
                x[r, pos] = rng.choice(SPECIALS, size=pos.size)
            else:            # a row of specials
                x[r] = rng.choice(SPECIALS, size=n)
    return x


def sine_window(n: int) -> np.ndarray:
    """2N values sin(pi (i + 1/2) / (2N)), float64 rounded once (kofft_amd.mdct.sine_window)"""
    return np.sin(np.pi * (np.arange(2 * n, dtype=np.float64) + 0.5) / (2 * n)).astype(F)


def cascade(rng, sections: int) -> np.ndarray:
    """A stable cascade as tests/sosfilt_oracle.cascade draws it (poles of radius 0.5 .. 0.9, numerators in [-1, 1)), from the case's rng."""
    r = rng.uniform(0.5, 0.9, sections)
    th = rng.uniform(0.2, 2.9, sections)
    sos = np.empty((sections, 6), F)
    sos[:, :3] = rng.uniform(-1, 1, (sections, 3))
    sos[:, 3] = 1
    sos[:, 4] = -2 * r * np.cos(th)
    sos[:, 5] = r * r
    return sos


def inputs(case: Case) -> dict:
    rng = np.random.default_rng(case.data_seed)
    g, fam = case.g, case.family
    if fam == "resample":
        return dict(x=_data(rng, (g["rows"], g["nx"]), case.specials), h=rng.uniform(-1, 1, g["nh"]).astype(F))
    if fam in ("sosfilt", "sosfilt_scan"):
        d = dict(x=_data(rng, (g["rows"], g["nx"]), case.specials), sos=cascade(rng, g["sections"]))
        d["zi"] = rng.uniform(-1, 1, (g["rows"], g["sections"], 2)).astype(F) if g["zi"] else None
        return d
    if fam == "convolve_bank":
        shape = (g["filters"], g["nh"])
        h = (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64) if g["complex_taps"] else rng.uniform(-1, 1, shape).astype(F)
        return dict(x=_data(rng, (g["rows"], g["nx"]), case.specials), h=h)
    if fam == "dct4":
        return dict(x=_data(rng, (g["rows"], g["n"]), case.specials))
    if fam == "mdct":
        w = sine_window(g["n"]) if g["window_kind"] == "sine" else rng.uniform(0.1, 1.0, 2 * g["n"]).astype(F)
        return dict(x=_data(rng, (g["rows"], g["nx"]), case.specials), window=w)
    x = _data(rng, (g["rows"] * g["frames"], g["n"]), case.specials).reshape(g["rows"], g["frames"], g["n"])
    return dict(x=x, window=sine_window(g["n"]) if case.data_seed % 2 else rng.uniform(0.1, 1.0, 2 * g["n"]).astype(F))


def strided(x: np.ndarray, stride: int) -> np.ndarray:
    """The rows as the MDCT sees them: (rows - 1) * stride + nx floats, NaN in the gaps."""
    rows, nx = x.shape
    flat = np.full((rows - 1) * stride + nx, np.nan, F)
    for r in range(rows):
        flat[r * stride:r * stride + nx] = x[r]
    return flat


# ---- expected values: each family's existing oracle -----------------------------------------------------------------------------------
def expected(case: Case, inp: dict) -> dict:
    """name -> array of every output of the (valid) call: 'out', and 'zf' for the filters where the call stores it.  The CPU oracle
    (oracle.pyoracle) must be built: convolve_bank and the DCT-IV family run their transforms on it."""
    g, fam = case.g, case.family
    with np.errstate(all="ignore"):
        if fam == "resample":
            from resample_oracle import resample_ref

            return dict(out=resample_ref(inp["x"], inp["h"], g["up"], g["down"], g["t0"], g["out_len"]))
        if fam == "sosfilt":
            from sosfilt_oracle import sosfilt_ref

            y, zf = sosfilt_ref(inp["sos"], inp["x"], inp["zi"], g["reverse"])
            return dict(out=y, zf=zf) if g["zf"] else dict(out=y)
        if fam == "sosfilt_scan":
            from sosfilt_scan_oracle import sosfilt_scan_ref

            y, zf = sosfilt_scan_ref(inp["sos"], inp["x"], g["chunk"], inp["zi"], g["reverse"])
            return dict(out=y, zf=zf) if g["zf"] else dict(out=y)
        if fam == "convolve_bank":
            from convolve_bank_oracle import convolve_bank_ref

            full = convolve_bank_ref(inp["x"], inp["h"], g["block"], g["correlate"], g["kind"])
            return dict(out=np.ascontiguousarray(full[:, :, g["out_first"]:g["out_first"] + g["out_len"]]))
        import mdct_oracle as mo

        if fam == "dct4":
            return dict(out=mo.dct4_ref(inp["x"]))
        if fam == "mdct":
            return dict(out=mo.mdct_ref(inp["x"], inp["window"], g["lead"], g["frames"]))
        full = mo.imdct_ref(inp["x"], inp["window"], g["scale"])
        return dict(out=np.ascontiguousarray(full[:, g["out_first"]:g["out_first"] + g["out_len"]]))


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
FLOAT64_MIN_VALUES = 8   # framed_expected.CONV_FLOAT64_MIN_VALUES: a window of fewer values has no meaningful relative error
RESAMPLE_ROWS_CHECKED = 4


def _window_rel(got64, want_full64, first, count):
    """framed_expected.conv_float64_error's measure: the L2 norm of the window's difference over the L2 norm of the whole float64 result
    scaled to the window's share of the values; None for a window of fewer than FLOAT64_MIN_VALUES values of a longer result."""
    full = want_full64.shape[-1]
    if count < min(FLOAT64_MIN_VALUES, full):
        return None
    den = float(np.linalg.norm(want_full64)) * np.sqrt(count / full)
    diff = float(np.linalg.norm(got64 - want_full64[..., first:first + count]))
    return diff / den if den else diff


def _dct4_f64(u64):
    """sum_i u[i] cos(pi / N (i + 1/2)(k + 1/2)) in float64: half of scipy's DCT-IV"""
    from scipy import fft as sfft

    return sfft.dct(u64, type=4, axis=-1) / 2.0


def _fold64(g):
    n = g.shape[-1] // 2
    h, q = n // 2, n + n // 2
    j, k = np.arange(h), np.arange(h, n)
    u = np.empty(g.shape[:-1] + (n,), np.float64)
    u[..., :h] = -g[..., q - 1 - j] - g[..., q + j]
    u[..., h:] = g[..., k - h] - g[..., q - 1 - k]
    return u


def _unfold64(v):
    n = v.shape[-1]
    h, q = n // 2, n + n // 2
    y = np.empty(v.shape[:-1] + (2 * n,), np.float64)
    y[..., :h] = v[..., h:]
    y[..., h:q] = -v[..., ::-1]
    y[..., q:] = -v[..., :h]
    return y


def float64_error(case: Case, inp: dict, out: dict, bounds: dict):
    """(error, bound) of a finite case's outputs against float64, in the measure and with the bound of the family's CPU test, which
    the caller hands in: bounds["resample"] = resample_oracle.forward_bound, ["sosfilt"] / ["sosfilt_scan"] the relative maximum error
    of test_sosfilt_cpu.py / test_sosfilt_scan_cpu.py, ["convolve_bank"](block) and ["dct"](n) the relative L2 bounds of
    test_convolve_bank_cpu.py and test_mdct_cpu.py.  None: nothing to hold (a window of a few values).  resample: the worst ratio of
    |out - float64 sum| to forward_bound over every output of up to RESAMPLE_ROWS_CHECKED rows, against 1."""
    g, fam = case.g, case.family
    got = np.asarray(out["out"])
    if fam == "resample":
        from resample_oracle import positions

        h64 = inp["h"].astype(np.float64)
        p, i0 = positions(g["up"], g["down"], g["t0"], g["out_len"])
        rows = sorted({0, 1 % g["rows"], g["rows"] // 2, g["rows"] - 1})[:RESAMPLE_ROWS_CHECKED]
        worst = 0.0
        for r in rows:
            x64 = inp["x"][r].astype(np.float64)
            acc = np.zeros(g["out_len"])
            for j in range(resample_terms(g["nh"], g["up"])):
                k, i = p + j * g["up"], i0 - j
                live = (k < g["nh"]) & (i >= 0) & (i < g["nx"])
                acc[live] += h64[k[live]] * x64[i[live]]
            b = bounds["resample"](inp["x"][r], inp["h"], g["up"], g["down"], g["t0"], g["out_len"])
            d = np.abs(got[r].astype(np.float64) - acc)
            assert (d[b == 0] == 0).all(), f"{case.describe()}: an output without terms is not +0"
            if (b > 0).any():
                worst = max(worst, float((d[b > 0] / b[b > 0]).max()))
        return worst, 1.0
    if fam in ("sosfilt", "sosfilt_scan"):
        from scipy import signal

        x64, sos64 = inp["x"].astype(np.float64), inp["sos"].astype(np.float64)
        zi = np.zeros((g["sections"], g["rows"], 2)) if inp["zi"] is None else inp["zi"].astype(np.float64).transpose(1, 0, 2)
        if g["reverse"]:
            x64 = x64[:, ::-1]
        want, _ = signal.sosfilt(sos64, x64, axis=-1, zi=zi)
        if g["reverse"]:
            want = want[:, ::-1]
        top = float(np.max(np.abs(want)))
        err = float(np.max(np.abs(got.astype(np.float64) - want)))
        return (err / top if top else err), bounds[fam]
    if fam == "convolve_bank":
        x64 = inp["x"].astype(np.float64)
        h64 = inp["h"].astype(np.complex128 if g["complex_taps"] else np.float64)
        op = (lambda a, b: np.correlate(a, b, "full")) if g["correlate"] else np.convolve
        want = np.stack([[op(r, t) for t in h64] for r in x64])
        if g["kind"] == "real":
            want = np.ascontiguousarray(want.real)
        elif g["kind"] == "magnitude":
            want = np.abs(want)
        g64 = got.astype(np.complex128 if g["kind"] == "complex" else np.float64)
        err = _window_rel(g64, want, g["out_first"], g["out_len"])
        return None if err is None else (err, bounds["convolve_bank"](g["block"]))
    import mdct_oracle as mo

    n = g["n"]
    if fam == "dct4":
        want = _dct4_f64(inp["x"].astype(np.float64))
        den = float(np.linalg.norm(want))
        return float(np.linalg.norm(got - want)) / den, bounds["dct"](n)
    if fam == "mdct":
        want = _dct4_f64(_fold64(mo.windowed_frames(inp["x"], inp["window"], g["lead"], g["frames"]).astype(np.float64)))
        den = float(np.linalg.norm(want))
        return float(np.linalg.norm(got - want)) / den, bounds["dct"](n)
    rows, frames = g["rows"], g["frames"]
    y = _unfold64(_dct4_f64(inp["x"].astype(np.float64))) * inp["window"].astype(np.float64)
    full = np.zeros((rows, (frames + 1) * n))
    for f in range(frames):
        full[:, f * n:(f + 2) * n] += y[:, f]
    full *= float(F(g["scale"]))
    err = _window_rel(got.astype(np.float64), full, g["out_first"], g["out_len"])
    return None if err is None else (err, bounds["dct"](n))
