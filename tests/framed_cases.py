"""The drawn cases of the frame-geometry fuzz (tests/test_gpu_framed_fuzz.py): a generator and a classifier, pure
Python and numpy -- nothing here imports torch or the library, so the coverage of the draw is checked without a GPU
(tests/test_framed_cases_cpu.py).

cases(seed) is deterministic from np.random.default_rng(31000 + seed): 8 framed cases and 3 convolve cases.  A framed case is ONE
geometry (win_len, hop, len, row_stride, rows) that every framed family is called on, each with its own frame count, form and route;
classify(case) names the classes it hits.  The frames per scratch chunk of every composed route are restated from the host sources
as formulas (the *_chunk functions below, each next to the line it restates); the CPU test asserts them on hand-worked shapes.

Size caps (the smallest shapes at which a seam can exist; nothing approaches a workload size): at most 2^20 complex points in
rows x frames x win_len, at most 2^13 frames in rows x frames (the Welch and mel oracles loop over frames or bins in Python), at most
2^18 pixels in a picture.  With a 1 MiB chunk a power-of-two picture with a row or a given maximum keeps 4 * (win_len / 2) bytes per
frame and would need more than 2^18 pixels for a seam, so such a case calls the picture family on fewer frames or not at all; the
running maximum (8 bytes per bin) and the Bluestein lengths (8 * win_len more per frame) seam inside the cap.  The fused Welch route
keeps only one partial per group of 32 frames in the scratch (4 * K bytes, 8 * K for a cross spectrum): under the caps its partials
never exceed 1 MiB, so the fused Welch route has no chunk seam of its own here; its pair with `seam_inside_row` is a case in which
another family's chunk seam falls inside a row while Welch runs fused on the same context."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

F = np.float32
SEEDS = 16
FRAMED_PER_SEED = 8
CONVOLVE_PER_SEED = 3

WINS = [1, 2, 3, 5, 15, 16, 31, 32, 33, 64, 128, 256, 400, 512, 1000, 1024, 2048, 4096, 8192]
MID_WINS = [w for w in WINS if 32 <= w <= 4096]
BIG_WINS = [256, 400, 512, 1000, 1024, 2048, 4096]  # a 1 MiB chunk is exceeded within the caps
MAX_POINTS = 1 << 20
MAX_FRAMES = 1 << 13
MAX_PIXELS = 1 << 18
GROUP = 32                       # KOFFT_HIP_WELCH_GROUP
CHUNK_DEFAULT = 512 << 20        # kScratchChunkDefaultBytes (host_layout.h)
CHUNK_1MB = 1 << 20              # KOFFT_HIP_SCRATCH_CHUNK_MB=1
FORMS = ["host", "dev", "dev_off"]
FRAME_FAMILIES = ["stft", "mags", "onesided", "mel", "mfcc", "picture", "welch", "csd"]
NUM_MEL = [1, 26, 40, 80, 128, 129]
FORMATS = [(8, 3), (8, 4), (16, 3)]
PALETTES = [0, 1, 2, 6]          # KOFFT_CMAP_FIRE, LEGACY, GRAY, RAINBOW
SAMPLE_RATE = 16000
BLOCKS = [2, 32, 64, 1024, 4096, 8192]
CONV_MAX_POINTS = 1 << 20        # rows * blocks * block of a convolve case

# the codes of include/kofft_hip.h
OK, MISMATCHED_LENGTHS, INVALID_VALUE = 0, 3, 6


def is_pow2(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@dataclass
class Case:
    """One framed geometry.  frames / forms: per family of FRAME_FAMILIES (a family missing from `frames` is not called)."""
    seed: int
    index: int
    win_len: int
    hop: int
    rows: int
    len: int
    row_stride: int
    frames: dict
    forms: dict
    ctx: str                      # "default" or "chunk1"
    welch_fused: int
    frontend_fused: int
    mfcc_fused: int
    transpose: int
    caller_window: bool
    specials: bool
    num_mel: int
    num_coeffs: int
    picture: dict                 # max_mode, mode, level, cmap, depth, channels, scale, layout
    welch_scale: float
    welch_double: bool
    data_seed: int
    release_after: int = -1       # kofft_hip_release_scratch after this many family calls (-1: never)
    stream_at: int = -1           # the family call that runs on a side stream (-1: none)
    kind: str = "framed"

    @property
    def required(self) -> int:
        return ceil_div(self.len, self.hop)

    @property
    def cap(self) -> int:
        return CHUNK_1MB if self.ctx == "chunk1" else CHUNK_DEFAULT

    def describe(self) -> str:
        return (f"seed={self.seed} case={self.index} win_len={self.win_len} hop={self.hop} len={self.len} row_stride={self.row_stride} "
                f"rows={self.rows} required={self.required} ctx={self.ctx} window={'caller' if self.caller_window else 'hann'} "
                f"specials={self.specials}")


@dataclass
class ConvCase:
    seed: int
    index: int
    block: int
    nh: int
    nx: int
    rows: int
    per_row: bool
    correlate: bool
    window: str                   # full, same, valid, inside, last
    out_first: int
    out_len: int
    fused: int
    form: str
    ctx: str
    data_seed: int
    kind: str = "convolve"

    @property
    def hop(self) -> int:
        return self.block - self.nh + 1

    @property
    def full(self) -> int:
        return self.nx + self.nh - 1

    @property
    def cap(self) -> int:
        return CHUNK_1MB if self.ctx == "chunk1" else CHUNK_DEFAULT

    def describe(self) -> str:
        return (f"seed={self.seed} case={self.index} family=convolve block={self.block} nh={self.nh} nx={self.nx} rows={self.rows} "
                f"per_row={self.per_row} correlate={self.correlate} window={self.window} out_first={self.out_first} out_len={self.out_len} "
                f"route={'fused' if conv_route(self) == 'fused' else conv_route(self)} form={self.form} ctx={self.ctx}")


# ---- the chunk arithmetic of the composed routes, restated ----------------------------------------------------------------------
def chunk_rows(cap_bytes: int, row_bytes: int, count: int) -> int:
    """scratch_chunk_rows (host_layout.h): cap / row bytes, at least 1, at most count; count 0: 0."""
    if count == 0:
        return 0
    chunk = cap_bytes // row_bytes if row_bytes else count
    return min(max(chunk, 1), count)


def kernels_cover(win_len: int) -> bool:
    """fused_len_ok<float> (host_common.hip.h): the STFT kernels take powers of two up to 2^14; every other length is composed
    (Bluestein) through win_len * 8 bytes of scratch per frame."""
    return is_pow2(win_len) and win_len <= 1 << 14


def picture_chunk(win_len: int, running: bool, cap: int, total: int) -> int:
    """k_picture_f32.hip, picture_dev: frame_bytes = 4 * (win_len / 2) (twice under the running maximum, which keeps the per-pixel
    maxima too) + 8 * win_len for a composed window length."""
    half = win_len // 2
    return chunk_rows(cap, half * 4 * (2 if running else 1) + (0 if kernels_cover(win_len) else win_len * 8), total)


def frontend_chunk(win_len: int, cap: int, total: int) -> int:
    """k_frontend_f32.hip, frontend_composed: 4 * (win_len / 2) + 8 * win_len for a composed window length."""
    return chunk_rows(cap, (win_len // 2) * 4 + (0 if kernels_cover(win_len) else win_len * 8), total)


def composed_stft_chunk(win_len: int, cap: int, total: int) -> int:
    """k_stft_rows.hip, composed_chunk: 8 * win_len per frame -- stft_rows, stft_magnitudes_rows and stft_onesided at a window length
    the kernels do not cover (the power-of-two lengths use no scratch: 0 means no chunk walk)."""
    return 0 if kernels_cover(win_len) else chunk_rows(cap, win_len * 8, total)


def welch_frames_walked(length: int, hop: int, frames: int) -> int:
    """k_welch_f32.hip, welch_dev: only the frames that can hold a sample are walked, at least one."""
    holding = (length - 1) // hop + 1 if length else 1
    return min(frames, holding)


def welch_chunk_end(t0: int, cap: int, frames: int, total: int) -> int:
    """welch_cut.h, welch_chunk_end: the last group seam at or before t0 + cap, or the end of t0's own group."""
    if total - t0 <= cap:
        return total
    e = t0 + cap
    r, f = divmod(e, frames)
    seam = r * frames + f // GROUP * GROUP
    if seam > t0:
        return seam
    r0, f0 = divmod(t0, frames)
    return r0 * frames + (frames if frames - f0 < GROUP else f0 + GROUP)


def welch_composed_cap(win_len: int, csd: bool, cap_bytes: int, total: int) -> int:
    """k_welch_f32.hip, welch_composed: per frame 8 * K bytes of one-sided spectrum (8 * win_len at a composed length; twice for
    the cross spectrum) plus its share of a group's partial, ceil(4 * vals / 32); never less than one group."""
    K = win_len // 2 + 1
    vals = K * (2 if csd else 1)
    fstride = K if kernels_cover(win_len) else win_len
    per_frame = fstride * 8 * (2 if csd else 1) + (vals * 4 + GROUP - 1) // GROUP
    cap = chunk_rows(cap_bytes, per_frame, total)
    if cap < GROUP:
        cap = min(GROUP, total)
    return cap


def welch_route(case: Case) -> str:
    """welch_use_fused: mode 0 never, mode 2 wherever the kernel exists (powers of two 64 .. 4096), mode 1 the same but 2048."""
    w = case.win_len
    fits = is_pow2(w) and 64 <= w <= 4096
    if case.welch_fused and fits and (case.welch_fused == 2 or w != 2048):
        return "fused"
    return "small-n" if w < 32 else "composed"


def frontend_route(case: Case) -> str:
    """frontend_use_fused: only mode 2, powers of two 64 .. 2048 with at most 128 filters."""
    w = case.win_len
    if case.frontend_fused == 2 and is_pow2(w) and 64 <= w <= 2048 and case.num_mel <= 128:
        return "fused"
    return "small-n" if w < 32 else "composed"


def mfcc_route(case: Case) -> str:
    """The MFCC stage behind a composed front end (kofft_hip_set_mfcc_fused): mode 1 up to 80 filters and 16 coefficients, mode 2 up
    to 128 filters."""
    if frontend_route(case) == "fused":
        return "in-frontend"
    if case.mfcc_fused == 2 and case.num_mel <= 128:
        return "fused"
    if case.mfcc_fused == 1 and case.num_mel <= 80 and case.num_coeffs <= 16:
        return "fused"
    return "composed"


def conv_route(c: ConvCase) -> str:
    """convolve_dev: blocks 32 .. 4096 fused unless switched off."""
    if c.fused and 32 <= c.block <= 4096:
        return "fused"
    return "small-n" if c.block < 32 else "composed"


def conv_window_blocks(c: ConvCase):
    """(first block, blocks) the window touches: s.b0 and s.nbw of convolve_dev."""
    b0 = c.out_first // c.hop
    return b0, (c.out_first + c.out_len - 1) // c.hop - b0 + 1


def seams(case: Case) -> dict:
    """family -> the flat frame indices t = row * frames + frame at which a scratch chunk of that family's route begins (0 excluded)."""
    out = {}
    w, cap = case.win_len, case.cap
    for fam in ("stft", "mags", "onesided"):
        if fam in case.frames:
            total = case.rows * case.frames[fam]
            chunk = composed_stft_chunk(w, cap, total)
            out[fam] = list(range(chunk, total, chunk)) if chunk else []
    for fam in ("mel", "mfcc"):
        if fam in case.frames:
            total = case.rows * case.frames[fam]
            if frontend_route(case) == "fused" or refusal(case, fam) is not None:
                out[fam] = []
            else:
                chunk = frontend_chunk(w, cap, total)
                out[fam] = list(range(chunk, total, chunk))
    if "picture" in case.frames and refusal(case, "picture") is None and w >= 2:
        total = case.rows * case.frames["picture"]
        chunk = picture_chunk(w, case.picture["max_mode"] == 1, cap, total)
        out["picture"] = list(range(chunk, total, chunk))
    for fam in ("welch", "csd"):
        if fam in case.frames:
            out[fam] = []
            if welch_route(case) != "fused":
                fr = welch_frames_walked(case.len, case.hop, case.frames[fam])
                total = case.rows * fr
                c = welch_composed_cap(w, fam == "csd", cap, total)
                t0 = welch_chunk_end(0, c, fr, total)
                while t0 < total:
                    out[fam].append(t0)
                    t0 = welch_chunk_end(t0, c, fr, total)
    return out


def seam_frames(case: Case, fam: str) -> int:
    """the frames per row that family's flat index counts with"""
    return welch_frames_walked(case.len, case.hop, case.frames[fam]) if fam in ("welch", "csd") else case.frames[fam]


def refusal(case: Case, fam: str):
    """The code include/kofft_hip.h documents for a family call of this case, or None where the call is valid."""
    # the STFT checks come first in every family: the frame count, where the family checks it (Welch and the device forms of stft_rows
    # never do; the one-sided family's frames are never drawn below required, so it has no branch here)
    if fam in ("mags", "mel", "mfcc", "picture") and case.frames[fam] < case.required:
        return MISMATCHED_LENGTHS
    if fam == "stft" and case.forms[fam] == "host" and case.frames[fam] < case.required:
        return MISMATCHED_LENGTHS
    if fam == "mfcc" and case.num_coeffs > case.num_mel:
        return INVALID_VALUE
    if fam == "picture" and case.picture["max_mode"] == 1 and case.picture["scale"] == 1:
        return INVALID_VALUE
    if fam == "picture" and case.picture["scale"] == 1 and case.win_len < 2:
        return INVALID_VALUE  # no bins, so no table: scale 1 with a null table is refused before the no-bins case is looked at
    return None


# ---- the classifier -----------------------------------------------------------------------------------------------------------------
def classify(case) -> set:
    if case.kind == "convolve":
        return _classify_conv(case)
    c = set()
    w, hop = case.win_len, case.hop
    c.add(f"welch:{welch_route(case)}")
    c.add(f"frontend:{frontend_route(case)}")
    c.add(f"mfcc:{mfcc_route(case)}")
    c.add(f"ctx:{case.ctx}")
    c.add("hop<win" if hop < w else "hop==win" if hop == w else "hop>win")
    if case.len < w:
        c.add("len<win")
    if any(case.frames[f] > case.required for f in ("stft", "mags", "onesided", "mel", "mfcc", "picture") if f in case.frames):
        c.add("frames>required")
    for fam in ("welch", "csd"):
        if case.frames[fam] < case.required:
            c.add("welch_frames<required")
        if case.frames[fam] > case.required:
            c.add("welch_frames>required")
        fr = welch_frames_walked(case.len, hop, case.frames[fam])
        groups = ceil_div(fr, GROUP)
        if fr % GROUP:
            c.add("last_group_short")
        if fr % GROUP == 1 and groups > 1:
            c.add("last_group_of_one")
        c.add("one_group" if groups == 1 else "many_groups")
    if case.rows > 1 and case.row_stride > case.len:
        c.add("stride_gap")
    if case.rows > 1:
        c.add("rows>1")
    s = seams(case)
    inside = boundary = False
    for fam, ts in s.items():
        fr = seam_frames(case, fam)
        for t in ts:
            if t % fr:
                inside = True
            else:
                boundary = True
    if inside:
        c.add("seam_inside_row")
    if boundary:
        c.add("seam_at_row_boundary")
    if not inside and not boundary:
        c.add("no_seam")
    for fam in ("welch", "csd"):  # the chunk capacity is no multiple of the group: welch_chunk_end had to step back to a seam
        if s[fam]:
            fr = welch_frames_walked(case.len, hop, case.frames[fam])
            cap = welch_composed_cap(w, fam == "csd", case.cap, case.rows * fr)
            prev = 0
            for t in s[fam]:
                if t != prev + cap:
                    c.add("seam_off_group")
                prev = t
    if not kernels_cover(w):
        c.add("bluestein")
    if w % 2:
        c.add("odd_win")
    if w < 32:
        c.add("small_win")
    if case.specials:
        c.add("specials")
    if case.caller_window:
        c.add("caller_window")
    if "picture" in case.frames:
        c.add(f"picture:max_mode{case.picture['max_mode']}")
    if any(refusal(case, fam) is not None for fam in case.frames):
        c.add("refusal")
    for fam in case.frames:
        c.add(f"form:{case.forms[fam]}")
    return c


def _classify_conv(c: ConvCase) -> set:
    out = {f"conv:{conv_route(c)}", f"conv_window:{c.window}", f"conv_form:{c.form}"}
    if c.per_row and c.rows > 1:
        out.add("conv_per_row")
    if c.correlate:
        out.add("conv_correlate")
    if c.hop == 1:
        out.add("conv_hop1")
    nb = ceil_div(c.full, c.hop)
    out.add("conv_one_block" if nb == 1 else "conv_many_blocks")
    if c.out_first % c.hop:
        out.add("conv_starts_inside_a_block")
    if (c.out_first + c.out_len) % c.hop and c.out_first + c.out_len != c.full:
        out.add("conv_ends_inside_a_block")
    # k_convolve_f32.hip, convolve_dev: the composed route keeps 8 * block bytes per (row, block) item of the window
    _, nbw = conv_window_blocks(c)
    if conv_route(c) != "fused" and chunk_rows(c.cap, c.block * 8, c.rows * nbw) < c.rows * nbw:
        out.add("conv_chunk_seam")
    return out


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _win_len(rng, big: bool) -> int:
    if big:
        return int(_pick(rng, BIG_WINS))
    return int(_pick(rng, MID_WINS)) if rng.random() < 0.67 else int(_pick(rng, WINS))


def _hop(rng, w: int) -> int:
    kind = int(rng.integers(0, 7))
    hop = [1, w // 4, w // 2, w - 1, w, w + 3, int(rng.integers(1, w + w // 2 + 2))][kind]
    return max(1, hop)


def _extra(rng, room: int) -> int:
    e = [0, 1, int(rng.integers(2, 41))][int(rng.integers(0, 3))]
    return max(0, min(e, room))


def _framed(rng, seed: int, index: int) -> Case:
    ctx = "chunk1" if rng.random() < 0.5 else "default"
    big = ctx == "chunk1" and rng.random() < 0.95
    w = _win_len(rng, big)
    # every sixth case of the 128 takes the next window length of the list in turn, finite and not empty: no length is left to chance,
    # and each has a float64 figure
    slot = seed * FRAMED_PER_SEED + index
    turn = slot % 6 == 0
    if turn:
        big, w = False, WINS[(slot // 6) % len(WINS)]
    hop = _hop(rng, w)
    if big and hop == 1 and rng.random() < 0.7:
        hop = max(1, w // 4)
    rows = int([1, 2, 3, 5, int(rng.integers(1, 41))][int(rng.integers(0, 5))])
    picture = dict(max_mode=int(rng.integers(0, 3)), mode=int(rng.integers(0, 2)), cmap=int(_pick(rng, PALETTES)), scale=int(rng.integers(0, 2)),
                   layout=int(rng.integers(0, 2)))
    picture["depth"], picture["channels"] = FORMATS[int(rng.integers(0, 3))]
    picture["level"] = [-80.0, 60.0][picture["mode"]]
    if picture["max_mode"] == 1 and picture["scale"] == 1 and rng.random() < 0.5:  # (the refusal stays in the draw, at half its weight)
        picture["scale"] = 0
    budget = max(1, min(MAX_FRAMES, MAX_POINTS // w))  # frames in rows x frames
    aligned = big and is_pow2(w) and 256 <= w <= 2048 and rng.random() < 0.3
    same_frames = None
    if aligned:
        # a seam of the running-maximum picture on a row boundary: chunk = 2^20 / (8 * (w / 2)) frames, frames = chunk / d, d < rows <= 2 d
        d = int(_pick(rng, [1, 2, 4]))
        rows = int(rng.integers(d + 1, 2 * d + 1))
        picture["max_mode"], picture["scale"] = 1, 0
        same_frames = (CHUNK_1MB // (8 * (w // 2))) // d
        assert rows * same_frames * w <= MAX_POINTS and rows * same_frames * (w // 2) <= MAX_PIXELS and rows * same_frames <= MAX_FRAMES
    rows = min(rows, budget)
    per_row = same_frames if aligned else max(1, budget // rows)  # the most frames a family may ask for
    room = min(40, per_row - 1)
    top = per_row - room                       # the largest `required`
    if aligned:
        nf = per_row - int(rng.integers(0, 3))
    elif big:
        nf = int(rng.integers(max(1, (3 * top) // 4), top + 1))
    else:
        nf = int(rng.integers(1, min(top, 130) + 1))
    r = rng.random()
    if r < 0.04 and not turn:
        length = 0
    elif r < 0.22 and w > 1 and not aligned:
        length = int(rng.integers(1, min(w - 1, nf * hop) + 1))          # shorter than the window
    elif r < 0.62 and hop > 1:
        length = (nf - 1) * hop + int(rng.integers(1, hop))                # the last frames run past the end of the row
    else:
        length = nf * hop
    required = ceil_div(length, hop)
    assert required <= per_row
    stride = length + [0, 1, int(rng.integers(2, 65))][int(rng.integers(0, 3))]
    frames = {}
    for fam in ("stft", "mags", "onesided", "mel", "mfcc", "picture"):
        frames[fam] = same_frames if aligned else max(1, required + _extra(rng, per_row - required))
    for fam in ("welch", "csd"):
        below = int(rng.integers(1, required)) if required > 1 else 1
        v = [1, 31, 32, 33, 64, 65, below, max(1, required), required + 1 + int(rng.integers(0, 8))][int(rng.integers(0, 9))]
        if big and rng.random() < 0.6:
            v = max(1, required)
        frames[fam] = max(1, min(v, per_row))
    caller_window = bool(rng.random() < 0.4)
    if caller_window or (big and not aligned and rng.random() < 0.5):
        frames.pop("mags")                      # stft_magnitudes_rows is Hann's; (a big case: one family less to pay for)
    if rows * frames["picture"] * (w // 2) > MAX_PIXELS:
        if rows * max(1, required) * (w // 2) <= MAX_PIXELS:
            frames["picture"] = max(1, required)
        else:
            frames.pop("picture")
    num_mel = int(_pick(rng, NUM_MEL))
    num_coeffs = int(_pick(rng, [1, 13, num_mel]))
    if num_coeffs > num_mel and rng.random() < 0.5:
        num_coeffs = num_mel
    forms = {fam: _pick(rng, FORMS) for fam in FRAME_FAMILIES}
    forms["istft"] = _pick(rng, FORMS)
    return Case(seed=seed, index=index, win_len=w, hop=hop, rows=rows, len=length, row_stride=stride, frames=frames, forms=forms, ctx=ctx,
                welch_fused=int(rng.integers(0, 3)), frontend_fused=int(rng.integers(0, 3)), mfcc_fused=int(rng.integers(0, 3)),
                transpose=int(rng.integers(0, 2)), caller_window=caller_window, specials=bool(rng.random() < 0.25) and not turn, num_mel=num_mel,
                num_coeffs=num_coeffs, picture=picture, welch_scale=float(F(rng.uniform(0.001, 2.0))), welch_double=bool(rng.random() < 0.5),
                data_seed=int(rng.integers(0, 1 << 31)))


def _convolve(rng, seed: int, index: int) -> ConvCase:
    # context, route and window take turns (4 and 5 are coprime: every combination over the 48 cases); the sizes are drawn
    slot = seed * CONVOLVE_PER_SEED + (index - FRAMED_PER_SEED)
    ctx, fused = ("chunk1" if slot % 2 else "default"), (slot // 2) % 2
    block = int(_pick(rng, BLOCKS))
    nh = max(1, int(_pick(rng, [1, 2, block // 2, block - 1, block])))
    rows = int(_pick(rng, [1, 3, 17]))
    # the composed route on the 1 MiB context: 17 rows as long as the caps allow, so that its 8 * block bytes per (row, block) fill more
    # than one chunk (not where the window is the last sample alone: one block per row)
    fill = ctx == "chunk1" and not fused and slot % 5 != 4
    if fill:
        rows = 17
    # the cap on rows * blocks * block: even nx == 1 takes ceil(nh / hop) blocks, so a long filter in a large block loses rows first, then
    # taps (block 4096: up to 4081 taps, a hop of 16; blocks up to 1024 keep block == nh, a hop of 1)
    most_blocks = CONV_MAX_POINTS // (rows * block)
    if nh > most_blocks * (block + 1) // (1 + most_blocks):
        rows, most_blocks = 1, CONV_MAX_POINTS // block
        nh = min(nh, most_blocks * (block + 1) // (1 + most_blocks))
    hop = block - nh + 1
    # (the two long kinds are drawn more often: only they fill more than one scratch chunk of the composed route)
    kind = int(rng.choice(7, p=[0.1, 0.1, 0.1, 0.1, 0.1, 0.2, 0.3]))
    nx = max(1, int([1, nh - 1, hop - 1, hop, hop + 1, 3 * hop + 7, int(rng.integers(1, 20001))][kind]))
    if fill:
        nx = 20000
    nx = max(1, min(nx, most_blocks * hop - nh + 1))
    full = nx + nh - 1
    window = ["full", "same", "valid", "inside", "last"][slot % 5]
    if window == "valid" and nx < nh:
        window = "full"
    if window == "full":
        first, count = 0, full
    elif window == "same":
        first, count = (nh - 1) // 2, nx
    elif window == "valid":
        first, count = nh - 1, nx - nh + 1
    elif window == "last":
        first, count = full - 1, 1
    else:
        first = int(rng.integers(0, full))
        if hop > 1 and first % hop == 0 and first + 1 < full:
            first += 1
        end = int(rng.integers(first + 1, full + 1))
        if hop > 1 and end % hop == 0 and end - 1 > first:
            end -= 1
        count = end - first
    return ConvCase(seed=seed, index=index, block=block, nh=nh, nx=nx, rows=rows, per_row=bool(rng.random() < 0.5), correlate=bool(rng.random() < 0.5),
                    window=window, out_first=first, out_len=count, fused=fused, form=_pick(rng, FORMS),
                    ctx=ctx, data_seed=int(rng.integers(0, 1 << 31)))


def cases(seed: int) -> list:
    rng = np.random.default_rng(31000 + seed)
    framed = [_framed(rng, seed, i) for i in range(FRAMED_PER_SEED)]
    conv = [_convolve(rng, seed, FRAMED_PER_SEED + i) for i in range(CONVOLVE_PER_SEED)]
    a, b = (int(v) for v in rng.choice(FRAMED_PER_SEED, size=2, replace=False))
    framed[a].release_after = int(rng.integers(1, 6))
    # the side stream goes to a family by turns over the seeds, whatever its form (the host forms stage through the context's stream too)
    target = FRAME_FAMILIES[seed % len(FRAME_FAMILIES)]
    b = next(k % FRAMED_PER_SEED for k in range(b, b + FRAMED_PER_SEED) if target in framed[k % FRAMED_PER_SEED].frames)
    framed[b].stream_at = family_order(framed[b]).index(target)
    # one family call per seed asks for fewer frames than ceil(len / hop): MISMATCHED_LENGTHS where the family checks the count, a
    # shorter valid output in the device form of stft_rows
    start = int(rng.integers(0, FRAMED_PER_SEED))
    for k in range(FRAMED_PER_SEED):
        c = framed[(start + k) % FRAMED_PER_SEED]
        short = [f for f in ("mags", "mel", "mfcc", "picture", "stft") if f in c.frames]
        if c.required >= 2:
            c.frames[short[seed % len(short)]] = c.required - 1 - (seed % 2 if c.required > 2 else 0)
            break
    return framed + conv


def stream_family(case: Case):
    """The family of the case that runs on a side stream, or None."""
    return family_order(case)[case.stream_at] if case.stream_at >= 0 else None


# ---- the inputs of a case -----------------------------------------------------------------------------------------------------------
def family_order(case: Case) -> list:
    """The families of the case in the order of its own rng."""
    fams = [f for f in FRAME_FAMILIES if f in case.frames]
    rng = np.random.default_rng(case.data_seed + 1)
    return [fams[i] for i in rng.permutation(len(fams))]


def inputs(case: Case) -> dict:
    """x, y [rows, len] float32 (y: the cross spectrum's second signal), window [win_len] (Hann: None), bins, max_in [rows], table."""
    import frontend_oracle as fo
    import mel_oracle as mo
    import spectrogram_oracle as so

    rng = np.random.default_rng(case.data_seed)
    x = fo.signal(rng, case.rows, case.len, special=case.specials)
    y = rng.standard_normal((case.rows, case.len)).astype(F)
    window = rng.uniform(0.1, 1.0, case.win_len).astype(F) if case.caller_window else None
    half = case.win_len // 2
    bins = np.array(mo.ref_bins(SAMPLE_RATE, half, case.num_mel), np.uint64)
    max_in = rng.uniform(0.25, 40.0, case.rows).astype(F)
    table = so.log_bin_map(half) if case.picture["scale"] == 1 and half >= 1 else None
    prefill = rng.standard_normal(4096).astype(F)  # the ISTFT outputs accumulate into a tiling of this
    return dict(x=x, y=y, window=window, bins=bins, max_in=max_in, table=table, prefill=prefill)


def strided(case: Case, x: np.ndarray) -> np.ndarray:
    """The rows as the call sees them: (rows - 1) * row_stride + len floats, NaN in the gaps."""
    n = (case.rows - 1) * case.row_stride + case.len
    flat = np.full(n, np.nan, F)
    for r in range(case.rows):
        flat[r * case.row_stride:r * case.row_stride + case.len] = x[r]
    return flat


def conv_inputs(c: ConvCase) -> dict:
    rng = np.random.default_rng(c.data_seed)
    x = rng.uniform(-1, 1, (c.rows, c.nx)).astype(F)
    h = rng.uniform(-1, 1, (c.rows, c.nh) if c.per_row and c.rows > 1 else (c.nh,)).astype(F)
    return dict(x=x, h=h)
