"""The drawn cases of the spectral fuzz (tests/test_gpu_spectral_fuzz.py): a generator and a classifier, pure Python and
numpy -- nothing here imports torch or the library, so the coverage of the draw is checked without a GPU
(tests/test_spectral_cases_cpu.py).  The oracles are imported where a function needs them.  Modelled on tests/filter_cases.py.

cases(seed) is deterministic from np.random.default_rng(35000 + seed): 10 cases, each ONE call of one family -- split32, split64
(kofft_hip_fft_split_c32 / _c64), czt, goertzel, dht, pfb_analysis or pfb_synthesis -- with a route, a form and a data kind.

Routes.  split: the value of set_split_fused.  czt: the value of set_czt_route; g["direct_tiled"] is the value of set_direct_tiled,
which the table route's sums obey (routes 0 and 2).  dht: the value of set_direct_tiled; g["table_device"] is the value of
set_dht_table_device.  pfb: the value of set_pfb_fused.  goertzel has no route: its forms stand twice in the list, so that its edge
classes get as many cases as the others'.

Forms.  host; dev; dev_off, every pointer one element off a 16-byte boundary (4 bytes, 8 for the f64 planes; the complex pfb spec and
out 8, as the header requires); inplace, where the header allows it: the split device form with in == out planes and dht's host form
with in == out; dev_oop: split's plain device form (the header also allows it in place, so the name says which); dev_unaligned
(pfb_analysis): dev_off with x two more bytes off, so no longer 4-byte aligned: the header sends it through the composed route.

Family, route and form take turns over the valid cases (COMBOS: 60 entries, every one at least twice in the 144 valid cases of the 16
seeds) and the cases of a seed keep that order, so what decides the state a context is in -- the chirp-Z keys and their order, the
Goertzel coefficient sets of the device calls, the Hartley lengths -- is a function of a family's turn and is the same whatever the
seeds draw; context (where the turn does not fix it), geometry and data are drawn.  One case per seed is a call the header refuses
(REFUSALS, one kind per seed), built as a valid case with one argument replaced: it carries the code.  One valid case per seed is
preceded by kofft_hip_release_scratch and one valid case runs on a side stream.

Size caps (the smallest shapes at which the kernels change behaviour; nothing approaches a workload size): split: batch * n <= 2^20;
czt: batch * n * m <= 2^24; goertzel: batch * n * nfreq <= 2^24; dht: n <= 2048 and batch * n <= 2^17 (the oracle's table costs 0.24 s
at n = 1024 and 3.3 s at 4096); pfb: rows * frames * M <= 2^20 and rows * nx <= 2^20 (synthesis: rows * full)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Optional

import numpy as np

F = np.float32
SEEDS = 16
PER_SEED = 10
VALID_PER_SEED = PER_SEED - 1
CHUNK_DEFAULT = 512 << 20        # kScratchChunkDefaultBytes (host_layout.h)
CHUNK_1MB = 1 << 20              # KOFFT_HIP_SCRATCH_CHUNK_MB=1
SPLIT_MAX = 1 << 20
CZT_MAX = 1 << 24
GOERTZEL_MAX = 1 << 24
DHT_MAX_N = 2048
DHT_MAX = 1 << 17
PFB_MAX = 1 << 20

# the codes of include/kofft_hip.h
OK, EMPTY_INPUT, MISMATCHED_LENGTHS, INVALID_HOP_SIZE, INVALID_VALUE, UNSUPPORTED, NULL = 0, 1, 3, 5, 6, -2, -3

SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.2e-38, 3e38, -3e38, np.inf, -np.inf, np.nan], F)  # test_gpu_rowwise_fuzz.py

FAMILIES = ["split32", "split64", "czt", "goertzel", "dht", "pfb_analysis", "pfb_synthesis"]
ROUTES = {"split32": [0, 1], "split64": [0, 1], "czt": [0, 1, 2], "goertzel": [0], "dht": [0, 1], "pfb_analysis": [0, 1, 2],
          "pfb_synthesis": [0, 1, 2]}
FORMS = {"split32": ["host", "dev_oop", "dev_off", "inplace"], "split64": ["host", "dev_oop", "dev_off", "inplace"],
         "czt": ["host", "dev", "dev_off"], "goertzel": ["host", "dev", "dev_off"], "dht": ["host", "dev", "dev_off", "inplace"],
         "pfb_analysis": ["host", "dev", "dev_off", "dev_unaligned"], "pfb_synthesis": ["host", "dev", "dev_off"]}
_ALL = [(fam, r, form) for fam in FAMILIES for r in ROUTES[fam] for form in FORMS[fam]] + [("goertzel", 0, form) for form in FORMS["goertzel"]]
COMBOS = [_ALL[i] for i in np.random.default_rng(34999).permutation(len(_ALL))]  # (a fixed shuffle: every seed holds several families)
VALID = SEEDS * VALID_PER_SEED


def _combo(v: int):
    return COMBOS[v % len(COMBOS)]


def _count(v: int, pred) -> int:
    """how many of the valid cases before the v-th satisfy pred(family, route, form)"""
    return sum(1 for u in range(v) if pred(*_combo(u)))


def _side_stream_families():
    """The family whose case runs on a side stream, per seed: of the families among the seed's valid cases (their turns are fixed by
    COMBOS) the one that had the side stream least often in the seeds before."""
    served = {fam: 0 for fam in FAMILIES}
    out = []
    for seed in range(SEEDS):
        here = {_combo(seed * VALID_PER_SEED + k)[0] for k in range(VALID_PER_SEED)}
        fam = min((f for f in FAMILIES if f in here), key=lambda f: served[f])
        served[fam] += 1
        out.append(fam)
    return out


SIDE_STREAM_FAMILY = _side_stream_families()

# (family, what) of the refused call of seed s
REFUSALS = [("split32", "n0"), ("czt", "n>4096"), ("czt", "overlap"), ("goertzel", "rate0"), ("goertzel", "nfreq>1024"), ("goertzel", "n0"),
            ("dht", "n>4096"), ("dht", "overlap"), ("pfb_analysis", "nh%m"), ("pfb_analysis", "bins>m"), ("pfb_synthesis", "hop0"),
            ("pfb_analysis", "lead"), ("pfb_analysis", "stride"), ("pfb_synthesis", "bins"), ("pfb_synthesis", "window"),
            ("pfb_analysis", "set_pfb_fused(3)")]
assert len(REFUSALS) == SEEDS

# split: the fused range's ends and their neighbours, the first length past it, the composed-only lengths
SPLIT_N = {"split32": [2, 32, 1 << 13, 1 << 14, 1 << 15, 1, 3, 12, 15, 1000, 4097], "split64": [2, 32, 1 << 12, 1 << 13, 1 << 14, 1, 3, 12, 15, 1000, 4097]}
SPLIT_FUSED_MAX = {"split32": 1 << 14, "split64": 1 << 13}   # max_log2<T>() of planar_impl.hip.h
SPLIT_COMPOSED_ONLY = [1, 3, 12, 15, 1000, 4097]
CZT_NM = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 4096]
CZT_SETS = ["dft", "zoom", "spiral", "a_zero", "grow", "dft_a0"]   # spectral_oracle.param_sets, and the DFT's w with a = 0
CZT_FINITE = ("dft", "zoom", "a_zero", "dft_a0")                   # test_spectral_cpu.FINITE_SETS: spiral underflows, grow overflows
CZT_BATCH = [1, 2, 3, 64, 65]
CZT_SLOTS = 4                                                      # kSpectralSlots
# the keys that come back (CZT_PLAN); their n are lengths of the context's dht cases
CZT_POOL = {"default": [(1000, 255, "dft"), (257, 2, "a_zero"), (2048, 64, "zoom")],
            "chunk1": [(1024, 63, "spiral"), (255, 256, "zoom"), (256, 1000, "dft_a0")]}
# the forced (n, m) of CZT_PLAN (None: drawn): the longest row, no samples (which takes no slot), 4096 bins
CZT_FORCED = {"default": [(4096, None), (0, None), (63, 4096)], "chunk1": [(4096, None), (0, None), (64, 4096)]}
GOERTZEL_N = [1, 2, 3, 4, 63, 64, 1000, 1023, 4096, 4099]
GOERTZEL_NFREQ = [1, 2, 255, 256, 257, 1024]
GOERTZEL_NFREQ_TURNS = [1, 1024, 1024, 1, 257, 2, 255, 256]   # of the cases outside the blocks below, by turns
GOERTZEL_MAX_FREQS = 1024
# the device calls of a context that repeat coefficient bits: turn 4 b + 0 .. 3 of the device forms is the whole set, the whole set
# again (nothing uploaded), its first `prefix` values (a different count: uploaded), the whole set (uploaded)
GOERTZEL_BLOCKS = [dict(ctx="default", n=1000, rate=8000.0, nfreq=257, prefix=255, seed=34990),
                   dict(ctx="chunk1", n=1023, rate=44100.0, nfreq=256, prefix=2, seed=34991)]
DHT_N = [2048, 256, 1000, 255, 257, 1024, 16, 17, 1, 2, 3]   # by turns; an even place runs on the default context, an odd one on the 1 MiB one
DHT_BATCH = [1, 2, 3, 63, 64, 65]
XPB = {5: 32, 6: 16, 7: 16, 8: 16, 9: 4, 10: 4, 11: 2, 12: 1}  # items per workgroup of the fused pfb kernels, by log2 M (test_gpu_pfb.py)
PFB_FUSED_M = [32 << i for i in range(8)]
PFB_OTHER_M = [1, 2, 16, 6, 240, 8192, 16384]
PFB_M = [32, 1, 64, 2, 128, 16, 256, 6, 512, 240, 1024, 8192, 2048, 16384, 4096]   # by turns
PFB_T = [1, 2, 3, 8]
PFB_WINDOWS = ["whole", "inside", "one", "last", "skip_chunks"]
# pfb synthesis on the 1 MiB context, the seams no ladder has.  Composed route (set_pfb_fused(0); 1 MiB / (8 M) frames a chunk): the
# first six of its cases.  Fused inverse (set_pfb_fused(1) or (2); 1 MiB / (4 M) frames a chunk): the first four.
SYNTH_COMPOSED = [dict(m=65536, taps=2, hop=16384, rows=1, frames=12, window="whole"),     # 2 frames a chunk, back = 7
                  dict(m=16384, taps=8, hop=8192, rows=2, frames=10, window="whole"),      # 8 a chunk, back = 15 clamped to 9
                  dict(m=16384, taps=1, hop=16389, rows=1, frames=12, window="inside"),    # D > nh across the seam at frame 8, a window
                  dict(m=4096, taps=2, hop=96, rows=1, frames=100, window="inside"),       # 32 a chunk, back = 85
                  dict(m=1024, taps=3, hop=1, rows=1, frames=200, window="skip_chunks"),   # 128 a chunk, back = 3071 clamped to 199
                  dict(m=2048, taps=1, hop=2053, rows=2, frames=70, window="inside")]      # D > nh, seams at frames 64 and 128 - 70, a window
SYNTH_FUSED = [dict(m=4096, taps=2, hop=96, rows=1, frames=130, window="whole"),           # 64 a chunk, back = 85
               dict(m=4096, taps=2, hop=1, rows=1, frames=70, window="inside"),            # back = 8191 clamped to 69
               dict(m=2048, taps=8, hop=100, rows=1, frames=300, window="inside"),         # 128 a chunk, back = 163
               dict(m=4096, taps=1, hop=4101, rows=1, frames=70, window="whole"),          # D > nh across the seam at frame 64
               dict(m=2048, taps=2, hop=1, rows=1, frames=140, window="whole"),            # 128 a chunk, back = 4095 clamped to 139
               dict(m=1024, taps=1, hop=1029, rows=1, frames=300, window="inside"),        # D > nh across the seam at frame 256, a window
               dict(m=512, taps=8, hop=7, rows=1, frames=700, window="last")]              # 512 a chunk, back = 585


def is_pow2(n: int) -> bool:
    return n >= 1 and n & (n - 1) == 0


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


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
    def device_form(self) -> bool:
        return self.form not in ("host",) and not (self.family == "dht" and self.form == "inplace")

    @property
    def cap(self) -> int:
        return CHUNK_1MB if self.ctx == "chunk1" else CHUNK_DEFAULT

    @property
    def real(self):
        return np.float64 if self.family == "split64" else F

    def describe(self) -> str:
        geo = " ".join(f"{k}={v}" for k, v in self.g.items())
        extra = f" refuse={self.refuse['what']}->{self.refuse['code']}" if self.refuse else ""
        return (f"seed={self.seed} case={self.index} family={self.family} route={self.route} form={self.form} ctx={self.ctx} "
                f"specials={self.specials} {geo}{extra}")


# ---- small arithmetic, restated from the host sources ---------------------------------------------------------------------------------
def chunk_rows(cap_bytes: int, row_bytes: int, count: int) -> int:
    """scratch_chunk_rows (host_layout.h): cap / row bytes, at least 1, at most count; count 0: 0."""
    if count == 0:
        return 0
    chunk = cap_bytes // row_bytes if row_bytes else count
    return min(max(chunk, 1), count)


def split_fused(case: Case) -> bool:
    """planar_fused_ok (planar_impl.hip.h): the switch on, n a power of two 2 .. 2^14 (f32) / 2^13 (f64)"""
    n = case.g["n"]
    return bool(case.route) and is_pow2(n) and 2 <= n <= SPLIT_FUSED_MAX[case.family]


def split_chunk(case: Case) -> int:
    """planar_composed_dev (planar_impl.hip.h): scratch_chunk_rows(scratch_chunk_bytes, n * sizeof(cpx<T>), batch)"""
    return chunk_rows(case.cap, case.g["n"] * (8 if case.family == "split32" else 16), case.g["batch"])


def pfb_fused(case: Case) -> bool:
    """pfb_fused_ok with pfb_use_fused (k_pfb_f32.hip): the switch not 0, M a power of two 32 .. 4096, x and h 4-byte aligned; then the
    switch at 2, or the inverse, or an analysis of M <= 1024."""
    m = case.g["m"]
    if case.route == 0 or not is_pow2(m) or m < 32 or m > 4096 or case.x_off2:
        return False
    return case.route == 2 or case.family == "pfb_synthesis" or m <= 1024


def analysis_chunk(case: Case) -> int:
    """pfb_analysis_items (k_pfb_f32.hip), the composed route: scratch_chunk_rows(scratch_chunk_bytes, m * sizeof(cpx<float>), items)"""
    g = case.g
    return chunk_rows(case.cap, g["m"] * 8, g["rows"] * g["frames"])


def synthesis_back(g) -> int:
    """kofft_hip_dev_pfb_synthesis_f32: back = (nh + d - 1) / d - 1, before its clamp to frames - 1"""
    return ceil_div(g["nh"], g["hop"]) - 1


def synthesis_chunk(case: Case) -> int:
    """kofft_hip_dev_pfb_synthesis_f32: scratch_chunk_rows(scratch_chunk_bytes, m * (fused ? sizeof(float) : sizeof(cpx<float>)), total)"""
    g = case.g
    return chunk_rows(case.cap, g["m"] * (4 if pfb_fused(case) else 8), g["rows"] * g["frames"])


def synthesis_full(g) -> int:
    return (g["frames"] - 1) * g["hop"] + g["nh"]


def synthesis_walk(case: Case) -> list:
    """The chunks of kofft_hip_dev_pfb_synthesis_f32's for_chunks: (t0, nt, pre, runs) -- pre the frames before t0 that are transformed
    again (min(t0 % frames, back), back clamped to frames - 1), runs False where the window touches none of the chunk's samples (frame f
    owns [f D, (f + 1) D) of its row's full, the last frame the rest)."""
    g = case.g
    frames, hop = g["frames"], g["hop"]
    total, full = g["rows"] * frames, synthesis_full(g)
    back = min(synthesis_back(g), frames - 1)
    chunk = synthesis_chunk(case)
    lo_w, hi_w = g["out_first"], g["out_first"] + g["out_len"]
    out = []
    for t0 in range(0, total, chunk):
        nt = min(chunk, total - t0)
        runs = False
        t = t0
        while t < t0 + nt:  # the pieces of frame_cut.h, row by row
            f = t % frames
            nf = min(frames - f, t0 + nt - t)
            end = full if f + nf == frames else (f + nf) * hop
            runs = runs or max(f * hop, lo_w) < min(end, hi_w)
            t += nf
        out.append((t0, nt, min(t0 % frames, back), runs))
    return out


def czt_params(g) -> tuple:
    """(wr, wi, ar, ai) as Python floats holding f32 values"""
    import spectral_oracle as so

    sets = so.param_sets(g["m"])
    w, a = (sets["dft"][0], 0j) if g["set"] == "dft_a0" else sets[g["set"]]
    (wr, wi), (ar, ai) = so._pair(w), so._pair(a)
    return float(wr), float(wi), float(ar), float(ai)


def czt_key(g):
    """the slot key of kofft_hip_dev_czt_f32: (n, m, the bits of w and a); None for n == 0, which takes no slot"""
    if g["n"] == 0:
        return None
    return (g["n"], g["m"]) + tuple(np.array(czt_params(g), F).view(np.uint32).tolist())


def goertzel_freqs(g) -> np.ndarray:
    """the call's target frequencies: the first nfreq of the set of g["freq_seed"]"""
    return np.random.default_rng(g["freq_seed"]).uniform(0, g["rate"] / 2, g["freq_count"]).astype(F)[:g["nfreq"]]


# ---- the classifier ---------------------------------------------------------------------------------------------------------------------
def classify(case: Case) -> set:
    fam, g = case.family, case.g
    c = {f"{fam}:route{case.route}:{case.form}", f"ctx:{case.ctx}", f"family:{fam}"}
    if case.refuse:
        return c | {"refusal", f"refusal:{fam}", f"refusal:{fam}:{case.refuse['what']}"}
    if case.specials:
        c.add("specials")
    if case.release_before:
        c.add("release_before")
    if case.side_stream:
        c.add("side_stream")
    if fam in ("split32", "split64"):
        n, batch = g["n"], g["batch"]
        top = SPLIT_FUSED_MAX[fam]
        c.add("split:fused" if split_fused(case) else "split:composed")
        c.add("split:inverse" if g["inverse"] else "split:forward")
        if n in (2, 32, top // 2, top):
            c.add("split:fused_range_end_or_neighbour")
        if n == 2 * top:
            c.add("split:just_past_the_fused_range")
        if n in SPLIT_COMPOSED_ONLY:
            c.add("split:composed_only_n")
        if n == 1:
            c.add("split:n1")
        if not is_pow2(n):
            c.add("split:bluestein")
        if n > 1 and abs(batch - CHUNK_1MB // (n * (8 if fam == "split32" else 16))) <= 1:
            c.add("split:batch_at_rows_per_chunk")
        if n > 1 and not split_fused(case) and split_chunk(case) < batch:
            c.add("split:chunk_seam")
    elif fam == "czt":
        n, m, batch = g["n"], g["m"], g["batch"]
        c.add(f"czt:set_{g['set']}")
        if n == 0:
            c.add("czt:n0")
        if m in (255, 256, 257):
            c.add("czt:m_at_256")
        if 4096 in (n, m):
            c.add("czt:longest")
        if m < 256 and abs(batch - 256 // m) <= 1:
            c.add("czt:batch_at_rows_per_block")
        if batch in (64, 65):
            c.add("czt:batch_at_64")
        if g["key_kind"] != "drawn":
            c.add(f"czt:key_{g['key_kind']}")
        if case.route != 1:
            c.add(f"czt:direct_tiled{g['direct_tiled']}")
    elif fam == "goertzel":
        n, nfreq, batch = g["n"], g["nfreq"], g["batch"]
        vec = n % 4 == 0 and case.form != "dev_off"   # goertzel_launch: n % 4 == 0 and a 16-byte aligned input
        c.add("goertzel:vector_loads" if vec else "goertzel:scalar_loads")
        c.add("goertzel:n%4==0" if n % 4 == 0 else "goertzel:n%4!=0")
        if nfreq in (255, 256, 257):
            c.add("goertzel:nfreq_at_256")
        if nfreq == 1:
            c.add("goertzel:one_frequency")
        if nfreq == GOERTZEL_MAX_FREQS:
            c.add("goertzel:most_frequencies")
        if abs(batch % max(256 // min(nfreq, 256), 1)) in (0, 1, 256 // min(nfreq, 256) - 1):
            c.add("goertzel:batch_at_rows_per_block")
        if g["coeff_kind"] != "drawn":
            c.add(f"goertzel:coeff_{g['coeff_kind']}")
    elif fam == "dht":
        n, batch = g["n"], g["batch"]
        c.add("dht:tiled_kernel" if case.route and n >= 64 and batch >= 64 else "dht:simple_kernel")  # direct_use_tiled
        c.add("dht:table_on_device" if g["table_device"] else "dht:table_on_host")
        if batch in (63, 64, 65):
            c.add("dht:batch_at_64")
        if n in (255, 256, 257):
            c.add("dht:n_at_256")
        if n <= 3:
            c.add("dht:tiny_n")
        if n == DHT_MAX_N:
            c.add("dht:longest")
        if n % 4:
            c.add("dht:n%4!=0")
    else:
        m, hop, nh = g["m"], g["hop"], g["nh"]
        fused = pfb_fused(case)
        short = "analysis" if fam == "pfb_analysis" else "synthesis"
        c.add(f"{short}:{'fused' if fused else 'composed'}")
        if m in PFB_OTHER_M or m > 4096:
            c.add("pfb:composed_only_m")
        if m in (32, 4096):
            c.add("pfb:fused_range_end")
        if not is_pow2(m):
            c.add("pfb:bluestein")
        if m == 1:
            c.add("pfb:m1")
        c.add(f"pfb:taps{nh // m}" if nh // m in PFB_T else "pfb:taps_other")
        c.add("pfb:hop_gt_nh" if hop > nh else "pfb:hop_gt_m" if hop > m else "pfb:hop_m" if hop == m else "pfb:hop_lt_m")
        if hop == 1:
            c.add("pfb:hop1")
        items = g["rows"] * g["frames"]
        if fused:
            xpb = XPB[m.bit_length() - 1]
            if xpb > 1 and items > xpb and items % xpb in (0, 1, xpb - 1):
                c.add("pfb:items_at_workgroup_multiple")
            if items > xpb:
                c.add("pfb:many_workgroups")
        if g["rows"] > 1:
            c.add("pfb:rows>1")
        if fam == "pfb_analysis":
            if case.x_off2 and case.route and is_pow2(m) and 32 <= m <= 4096 and (case.route == 2 or m <= 1024):
                c.add("analysis:off_alignment_composed")
            if case.route == 1 and is_pow2(m) and 2048 <= m <= 4096:
                c.add("analysis:measured_choice_composed")
            lead = g["lead"]
            c.add("analysis:lead_0" if lead == 0 else "analysis:lead_nh-1" if lead == nh - 1 else "analysis:lead_nh-hop" if lead == nh - hop else "analysis:lead_other")
            past = sum(1 for f in range(g["frames"]) if f * hop - lead >= g["nx"])
            if past:
                c.add("analysis:frames_past_the_end")
            if g["rows"] > 1 and g["row_stride"] > g["nx"]:
                c.add("analysis:stride_gap")
            c.add("analysis:bins_1" if g["bins"] == 1 and m > 1 else "analysis:bins_m" if g["bins"] == m else "analysis:bins_one_sided")
            if not fused:
                chunk = analysis_chunk(case)
                if chunk < items:
                    c.add("analysis:chunk_seam")
                if abs(items - CHUNK_1MB // (8 * m)) <= 1 and case.ctx == "chunk1":
                    c.add("analysis:items_at_chunk")
        else:
            c.add("synthesis:bins_m" if g["bins"] == m else "synthesis:bins_one_sided")
            c.add("synthesis:scale_1" if g["scale"] == 1.0 else "synthesis:scale_other")
            c.add(f"synthesis:window_{g['window']}")
            walk = synthesis_walk(case)
            how = "fused" if fused else "composed"
            if len(walk) > 1:
                chunk, back = synthesis_chunk(case), synthesis_back(g)
                c.add("synthesis:chunk_seam")
                if any(t0 % g["frames"] for t0, _, _, _ in walk):
                    c.add("synthesis:seam_inside_a_row")
                    if chunk < min(back, g["frames"] - 1):
                        c.add(f"synthesis:{how}:chunk_shorter_than_back")
                    if back > g["frames"] - 1:
                        c.add(f"synthesis:{how}:back_clamped")
                    if hop > nh:
                        c.add(f"synthesis:{how}:hop_gt_nh_across_a_seam")
                        if g["window"] != "whole":
                            c.add("synthesis:seam_window_and_hop_gt_nh")
                if not all(runs for _, _, _, runs in walk):
                    c.add("synthesis:chunk_left_out")
    return c


# ---- the generator ------------------------------------------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _dht_ctx(turn: int) -> str:
    return ["default", "chunk1"][(turn + turn // len(DHT_N)) % 2]


def _split(rng, fam, route, turn):
    size = 8 if fam == "split32" else 16
    ns = SPLIT_N[fam]
    n = ns[turn % len(ns)]
    ctx = None
    if turn % 4 == 3:  # a batch within one of the rows per 1 MiB chunk, on that context; with the fused route on, a length it does not take
        if route:
            n = [1000, 4097, ns[4], 12][(turn // 4) % 4]
        elif n == 1:
            n = 3
        batch = max(1, CHUNK_1MB // (n * size) + [1, 0, 1, -1][(turn // 4) % 4])
        ctx = "chunk1"
    else:
        batch = [1, 2, 3][turn % 4]
        if route and turn % 2 == 0:  # (the fused route on: every second of its cases a length it takes, the range's ends and their neighbours)
            n = ns[(turn // 2) % 4]
    assert batch * n <= SPLIT_MAX
    return dict(n=n, batch=batch, inverse=(turn + turn // 4) % 2), ctx


def _czt_batch(rng, n, m, turn):
    cands = list(CZT_BATCH) + ([256 // m - 1, 256 // m, 256 // m + 1] if m < 256 else [])
    cands = [b for b in cands if b >= 1 and b * max(n, 1) * m <= CZT_MAX] or [1]
    return int(cands[turn % len(cands)] if rng.random() < 0.6 else _pick(rng, cands))


CZT_PLAN = ["key0", "key1", "key2", "forced0", "dht_length", "key0", "key1", "forced1", "drawn", "key2", "forced2"]
CZT_QUIET = 7   # the first cases of a context's plan, up to the second key that comes back: no release_scratch on that context in between


def _czt(rng, route, turn):
    """The context and the key are the turn's: CZT_PLAN on the default context, then on the 1 MiB one.  A context's three keys of
    CZT_POOL each come back after four other keys, so after their eviction from the four slots; the forced lengths; the length of one
    of the context's dht cases (on the table route the same direct kernels run both); a drawn pair."""
    ctx = ["default", "chunk1"][(turn // len(CZT_PLAN)) % 2]
    what = CZT_PLAN[turn % len(CZT_PLAN)]
    lap = turn // (2 * len(CZT_PLAN)) + (turn % len(CZT_PLAN)) // 5
    kind, batch = "drawn", None
    name = ["dft_a0", "grow", "spiral", "a_zero", "dft", "zoom"][turn % 6]   # (of the cases that bring no key of their own)
    if what.startswith("key"):
        n, m, name = CZT_POOL[ctx][int(what[3:])]
        edge = 256 // m + [1, 0, -1][lap % 3] if m < 256 else 3  # (route 1 takes 256 / m rows a workgroup)
        kind, batch = "that_comes_back", [edge, 64, 65][(int(what[3:]) + lap) % 3]
    elif what.startswith("forced"):
        n, m = CZT_FORCED[ctx][int(what[6:])]
        m = int(_pick(rng, CZT_NM[1:]) if m is None else m)
    elif what == "dht_length":
        lengths = [v for i, v in enumerate(DHT_N) if v >= 16 and _dht_ctx(i) == ctx]
        n = lengths[lap % len(lengths)]
        m = int(_pick(rng, [1, 2, 63, 64, 65, 255, 256, 257, 1000]))
        kind, batch = "dht_length", [9, 64][lap % 2]
    else:
        n, m = int(_pick(rng, CZT_NM)), int(_pick(rng, CZT_NM[1:]))
    if batch is None or batch * n * m > CZT_MAX:
        batch = _czt_batch(rng, n, m, turn)
    return dict(n=n, m=m, batch=batch, set=name, direct_tiled=int(rng.integers(0, 2)), key_kind=kind), ctx


def quiet_contexts(seed: int) -> set:
    """The f32 contexts that get no release_scratch before a case of this seed: those whose chirp-Z plan is among its first CZT_QUIET
    cases somewhere in the seed, or between two of them."""
    quiet = set()
    for b, ctx in enumerate(["default", "chunk1"]):
        first, last = b * len(CZT_PLAN), b * len(CZT_PLAN) + CZT_QUIET - 1
        turns = [_count(v, lambda f, r, fo: f == "czt") for v in (seed * VALID_PER_SEED, (seed + 1) * VALID_PER_SEED)]
        if turns[0] <= last and turns[1] > first:   # (the seed's chirp-Z turns [turns[0], turns[1]) meet [first, last], or lie between)
            quiet.add(ctx)
    return quiet


def _goertzel_batch(rng, n, nfreq):
    rpb = 256 // min(nfreq, 256)
    most = max(1, GOERTZEL_MAX // (n * nfreq))
    return max(1, min(int(rng.integers(1, 3)) * rpb + int(rng.integers(-1, 2)), most))


def _goertzel(rng, form, turn, dev_turn):
    if form != "host" and dev_turn < 4 * len(GOERTZEL_BLOCKS):
        b, pos = GOERTZEL_BLOCKS[dev_turn // 4], dev_turn % 4
        nfreq = b["prefix"] if pos == 2 else b["nfreq"]
        kind = ["first", "repeat", "prefix", "again"][pos]
        return dict(n=b["n"], batch=_goertzel_batch(rng, b["n"], nfreq), nfreq=nfreq, rate=b["rate"], freq_seed=b["seed"], freq_count=b["nfreq"],
                    coeff_kind=kind), b["ctx"]
    j = turn - min(dev_turn, 4 * len(GOERTZEL_BLOCKS))  # the cases outside the blocks before this one
    nfreq = int(GOERTZEL_NFREQ_TURNS[j % len(GOERTZEL_NFREQ_TURNS)])
    n = int(_pick(rng, [v for v in GOERTZEL_N if v * nfreq <= GOERTZEL_MAX]))
    return dict(n=n, batch=_goertzel_batch(rng, n, nfreq), nfreq=nfreq, rate=float(_pick(rng, [8000.0, 44100.0, 1.0])),
                freq_seed=int(rng.integers(0, 1 << 31)), freq_count=nfreq, coeff_kind="drawn"), None


def _dht(rng, turn):
    n = DHT_N[turn % len(DHT_N)]
    cands = [b for b in DHT_BATCH if b * n <= DHT_MAX]
    edge = [b for b in cands if b >= 63]  # (the tiled kernel takes 64 rows and more of 64 outputs and more)
    batch = int(_pick(rng, edge) if n >= 64 and rng.random() < 0.7 else _pick(rng, cands))
    return dict(n=n, batch=batch, table_device=int(rng.integers(0, 2))), _dht_ctx(turn)


def _pfb_m(rng, route, form, turn, analysis=False):
    m = PFB_M[turn % len(PFB_M)]
    if form == "dev_unaligned" and route:  # a size the fused kernel would take, so that the alignment alone decides
        m = int(_pick(rng, PFB_FUSED_M[:6] if route == 1 else PFB_FUSED_M))
    elif analysis and route == 1 and turn % 3 == 0:  # the measured choice: a fused kernel exists and the composed route runs
        m = [2048, 4096][(turn // 3) % 2]
    return m


def _pfb_items(rng, m, fused, ctx, turn, bytes_per):
    """(items, kind): within one of a multiple of the fused kernel's items per workgroup; on the composed route of the 1 MiB context,
    by turns, within one of the items per chunk; a few otherwise"""
    if fused:
        return max(1, int(rng.integers(1, 4)) * XPB[m.bit_length() - 1] + int(rng.integers(-1, 2))), "workgroup"
    if ctx == "chunk1" and turn % 2 == 0:
        return max(1, CHUNK_1MB // (bytes_per * m) + [1, 0, 1, -1][(turn // 2) % 4]), "chunk"
    return int(rng.integers(1, 13)), "few"


def _pfb_rows(rng, items):
    return int(_pick(rng, [r for r in (1, 1, 2, 3, 5) if items % r == 0]))


def _analysis(rng, route, form, turn, ctx):
    m = _pfb_m(rng, route, form, turn, analysis=True)
    probe = Case(0, 0, "pfb_analysis", route, form, ctx, False, 0, dict(m=m))
    fused = pfb_fused(probe)
    if not fused and turn % 4 == 0:  # (the items per chunk need the 1 MiB context)
        ctx = "chunk1"
    for _ in range(400):
        taps = int(_pick(rng, PFB_T))
        nh = taps * m
        hop = max(1, int(_pick(rng, [1, m // 2, m - 3, m, m + 7, nh + 5])))
        lead = int(_pick(rng, [0, max(nh - hop, 0), nh - 1]))
        items, kind = _pfb_items(rng, m, fused, ctx, turn, 8)
        rows = _pfb_rows(rng, items)
        frames = items // rows
        covered = frames - int(_pick(rng, [0, 0, 1, 2]))  # up to two frames past the row's end
        hi = covered * hop - lead                         # frame `covered` is the first that holds no sample: nx <= hi
        if covered < 1 or hi < 1:
            continue
        nx = int(rng.integers(max(1, (covered - 1) * hop - lead + 1), hi + 1))
        stride = nx + int([0, 1, int(rng.integers(2, 65))][int(rng.integers(0, 3))])
        if rows * frames * m > PFB_MAX or rows * stride > PFB_MAX or rows * frames * nh > 8 * PFB_MAX:
            continue
        bins = max(1, min(m, int(_pick(rng, [1, m // 2 + 1, m]))))
        return dict(m=m, nh=nh, hop=hop, lead=lead, rows=rows, nx=nx, row_stride=stride, frames=frames, bins=bins, items_kind=kind), ctx
    raise AssertionError(f"no analysis geometry for M={m} route={route} form={form} ctx={ctx}")


def _window(rng, kind, full, hop, skip_from):
    """(kind, out_first, out_len); skip_from: the first sample behind the first chunk's (None: the call has one chunk)"""
    if kind == "skip_chunks" and (skip_from is None or skip_from >= full):
        kind = "inside"
    if kind == "inside" and full < 3:
        kind = "whole"
    if kind == "whole":
        return kind, 0, full
    if kind == "last":
        return kind, full - 1, 1
    if kind == "one":
        return kind, int(rng.integers(0, full)), 1
    if kind == "skip_chunks":
        first = int(rng.integers(skip_from, full))
    else:
        first = int(rng.integers(1, full - 1))
        if hop > 1 and first % hop == 0:  # (starting inside a hop block)
            first += 1
    return kind, first, int(rng.integers(1, full - first + 1))


def _synthesis(rng, route, form, turn, ctx, k_route):
    special = None
    if route == 0 and k_route < len(SYNTH_COMPOSED):
        special = SYNTH_COMPOSED[k_route]
    elif route and k_route < len(SYNTH_FUSED):
        special = SYNTH_FUSED[k_route]
    want = PFB_WINDOWS[turn % len(PFB_WINDOWS)]
    if special:
        ctx = "chunk1"
        m, taps, hop, rows, frames, want = (special[k] for k in ("m", "taps", "hop", "rows", "frames", "window"))
        nh, kind = taps * m, "seam"
    else:
        m = _pfb_m(rng, route, form, turn)
        if want == "skip_chunks":
            ctx = "chunk1"
    probe = Case(0, 0, "pfb_synthesis", route, form, ctx, False, 0, dict(m=m))
    fused = pfb_fused(probe)
    per = CHUNK_1MB // ((4 if fused else 8) * m)          # frames per chunk on the 1 MiB context
    for _ in range(400):
        if not special:
            taps = int(_pick(rng, PFB_T))
            nh = taps * m
            hop = max(1, int(_pick(rng, [1, m // 2, m - 3, m, m + 7, nh + 5])))
            if want == "skip_chunks":                     # one row of a little more than two chunks
                rows, frames, kind = 1, 2 * per + int(rng.integers(1, 4)), "two_chunks"
            else:
                items, kind = _pfb_items(rng, m, fused, ctx, turn, 4 if fused else 8)
                rows = _pfb_rows(rng, items)
                frames = items // rows
        full = (frames - 1) * hop + nh
        if rows * frames * m > PFB_MAX or rows * full > PFB_MAX:
            assert not special, special
            continue
        skip_from = per * hop if ctx == "chunk1" and rows == 1 and frames > per else None
        window, first, count = _window(rng, want, full, hop, skip_from)
        bins = m if m % 2 or m < 2 or rng.random() < 0.5 else m // 2 + 1
        scale = 1.0 if rng.random() < 0.4 else float(F(rng.uniform(0.05, 1.5)))
        return dict(m=m, nh=nh, hop=hop, rows=rows, frames=frames, bins=bins, scale=scale, out_first=first, out_len=count, window=window,
                    items_kind=kind), ctx
    raise AssertionError(f"no synthesis geometry for M={m} route={route} form={form} ctx={ctx}")


def _draw(rng, seed, v, fam, route, form) -> Case:
    """the v-th valid case (v counts over all seeds); a refused case is drawn as the valid case of a v of its own"""
    turn = _count(v, lambda f, r, fo: f == fam)
    ctx = "chunk1" if rng.random() < 0.5 else "default"
    fixed = None
    if fam in ("split32", "split64"):
        g, fixed = _split(rng, fam, route, turn)
    elif fam == "czt":
        g, fixed = _czt(rng, route, turn)
    elif fam == "goertzel":
        g, fixed = _goertzel(rng, form, turn, _count(v, lambda f, r, fo: f == "goertzel" and fo != "host"))
    elif fam == "dht":
        g, fixed = _dht(rng, turn)
    elif fam == "pfb_analysis":
        g, fixed = _analysis(rng, route, form, turn, ctx)
    else:
        g, fixed = _synthesis(rng, route, form, turn, ctx, _count(v, lambda f, r, fo: f == fam and bool(r) == bool(route)))
    return Case(seed=seed, index=-1, family=fam, route=route, form=form, ctx=fixed or ctx, specials=bool(rng.random() < 0.25),
                data_seed=int(rng.integers(0, 1 << 31)), g=g)


def _refusal(case: Case, what: str) -> dict:
    """The arguments that turn the valid call into one the header refuses, and the code it names for them.  overlap: the output
    pointer is the input's (device form; the check comes after the null checks, so it needs a context).  setter: no call of the family
    at all, kofft_hip_set_pfb_fused(ctx, 3)."""
    g = case.g
    if what == "n0":
        return dict(what=what, code=EMPTY_INPUT, args=dict(n=0))
    if what == "n>4096":
        return dict(what=what, code=UNSUPPORTED, args=dict(n=4097))
    if what == "overlap":
        return dict(what=what, code=INVALID_VALUE, args={}, overlap=True)
    if what == "rate0":
        return dict(what=what, code=INVALID_VALUE, args=dict(rate=[0.0, -1.0][case.seed % 2]))
    if what == "nfreq>1024":
        return dict(what=what, code=UNSUPPORTED, args=dict(nfreq=GOERTZEL_MAX_FREQS + 1))
    if what == "nh%m":
        return dict(what=what, code=INVALID_VALUE, args=dict(nh=g["nh"] + 1))
    if what == "bins>m":
        return dict(what=what, code=INVALID_VALUE, args=dict(bins=g["m"] + 1))
    if what == "hop0":
        return dict(what=what, code=INVALID_HOP_SIZE, args=dict(hop=0))
    if what == "lead":
        return dict(what=what, code=INVALID_VALUE, args=dict(lead=g["nh"]))
    if what == "stride":     # rows > 1 and row_stride < nx
        return dict(what=what, code=INVALID_VALUE, args=dict(rows=max(2, g["rows"]), row_stride=g["nx"] - 1))
    if what == "bins":       # neither M nor M / 2 + 1
        return dict(what=what, code=INVALID_VALUE, args=dict(bins=g["m"] - 1))
    if what == "window":     # out_first + out_len > full
        return dict(what=what, code=MISMATCHED_LENGTHS, args=dict(out_first=synthesis_full(g) - g["out_len"] + 1))
    if what == "set_pfb_fused(3)":
        return dict(what=what, code=INVALID_VALUE, args={}, setter=("kofft_hip_set_pfb_fused", 3))
    raise KeyError(what)


def _refusable(case: Case, what: str) -> bool:
    """the replaced argument breaks exactly one check of the header"""
    g = case.g
    if what == "overlap":
        return g["n"] >= 1 and g["batch"] >= 1 and g.get("m", 1) >= 1
    if what == "nh%m":
        return g["m"] >= 2
    if what == "bins":
        return g["m"] >= 8
    return True


def cases(seed: int) -> list:
    rng = np.random.default_rng(35000 + seed)
    out = []
    for k in range(VALID_PER_SEED):
        v = seed * VALID_PER_SEED + k
        out.append(_draw(rng, seed, v, *_combo(v)))
    fam, what = REFUSALS[seed]
    form = "dev" if "dev" in FORMS[fam] else "dev_oop"
    if what != "overlap":
        form = _pick(rng, [f for f in FORMS[fam] if f not in ("inplace", "dev_unaligned")])
    for attempt in range(64):  # a valid case of a turn past every real one (so none of the fixed sequences), redrawn until the replaced argument breaks one check only
        bad = _draw(rng, seed, VALID + 60 * attempt + seed, fam, int(_pick(rng, ROUTES[fam])), form)
        if _refusable(bad, what):
            break
    bad.specials = False
    bad.refuse = _refusal(bad, what)
    out.insert(int(rng.integers(0, len(out) + 1)), bad)
    for i, c in enumerate(out):
        c.index = i
    quiet = quiet_contexts(seed)
    _pick(rng, [c for c in out[1:] if not c.refuse and (c.ctx not in quiet or c.family == "split64")]).release_before = True
    next(c for c in out if not c.refuse and c.family == SIDE_STREAM_FAMILY[seed]).side_stream = True
    return out


# ---- the call's scalar arguments --------------------------------------------------------------------------------------------------------
def call_args(case: Case) -> dict:
    """The scalar arguments of the C call by name, the refused case's replacements applied."""
    g = case.g
    fam = case.family
    if fam in ("split32", "split64"):
        a = dict(n=g["n"], batch=g["batch"], inverse=g["inverse"])
    elif fam == "czt":
        wr, wi, ar, ai = czt_params(g)
        a = dict(n=g["n"], m=g["m"], wr=wr, wi=wi, ar=ar, ai=ai, batch=g["batch"])
    elif fam == "goertzel":
        a = dict(n=g["n"], batch=g["batch"], rate=g["rate"], nfreq=g["nfreq"])
    elif fam == "dht":
        a = dict(n=g["n"], batch=g["batch"])
    elif fam == "pfb_analysis":
        a = {k: g[k] for k in ("rows", "nx", "row_stride", "nh", "m", "hop", "lead", "frames", "bins")}
    else:
        a = {k: g[k] for k in ("rows", "frames", "bins", "nh", "m", "hop", "scale", "out_first", "out_len")}
    if case.refuse:
        a.update(case.refuse["args"])
    return a


ENTRY = {"split32": "fft_split_c32", "split64": "fft_split_c64", "czt": "czt_f32", "goertzel": "goertzel_f32", "dht": "dht_f32",
         "pfb_analysis": "pfb_analysis_f32", "pfb_synthesis": "pfb_synthesis_f32"}


def invoke(fn, ctx, case: Case, p: dict, host: bool) -> int:
    """Call the family's C entry `fn` (host: its host form, which for split takes two planes; else four) with the pointers p."""
    import ctypes as C

    a = call_args(case)
    fam = case.family
    if fam in ("split32", "split64"):
        if host:
            return fn(ctx, p["re"], p["im"], a["n"], a["batch"], a["inverse"])
        return fn(ctx, p["re"], p["im"], p["re_out"], p["im_out"], a["n"], a["batch"], a["inverse"])
    if fam == "czt":
        return fn(ctx, p["x"], p["out"], a["n"], a["m"], a["wr"], a["wi"], a["ar"], a["ai"], a["batch"])
    if fam == "goertzel":
        return fn(ctx, p["x"], p["out"], a["n"], a["batch"], C.c_float(a["rate"]), p["freqs"], a["nfreq"])
    if fam == "dht":
        return fn(ctx, p["x"], p["out"], a["n"], a["batch"])
    if fam == "pfb_analysis":
        return fn(ctx, p["x"], a["rows"], a["nx"], a["row_stride"], p["h"], a["nh"], a["m"], a["hop"], a["lead"], p["out"], a["frames"], a["bins"])
    return fn(ctx, p["x"], a["rows"], a["frames"], a["bins"], p["h"], a["nh"], a["m"], a["hop"], C.c_float(a["scale"]), p["out"], a["out_first"],
              a["out_len"])


def header_violations(case: Case) -> list:
    """Every precondition of the family's header block that the call breaks (empty: a valid call)."""
    a = call_args(case)
    fam = case.family
    bad = []
    if case.refuse and case.refuse.get("overlap"):
        bad.append("device in and out overlap")
    if case.refuse and case.refuse.get("setter"):
        bad.append("a route the setter does not know")
    if fam in ("split32", "split64"):
        if a["n"] == 0:
            bad.append("n == 0")
    elif fam == "czt":
        if a["n"] > 4096 or a["m"] > 4096:
            bad.append("n or m > 4096")
    elif fam == "goertzel":
        if a["n"] == 0:
            bad.append("n == 0")
        if a["rate"] <= 0:
            bad.append("sample_rate <= 0")
        if a["nfreq"] > GOERTZEL_MAX_FREQS or a["n"] > 1 << 26:
            bad.append("nfreq > 1024 or n > 2^26")
    elif fam == "dht":
        if a["n"] > 4096:
            bad.append("n > 4096")
    else:
        if a["m"] == 0 or a["nh"] == 0:
            bad.append("M or nh == 0")
        elif a["nh"] % a["m"]:
            bad.append("nh % M != 0")
        if a["bins"] == 0 or a["bins"] > a["m"]:
            bad.append("bins == 0 or bins > M")
        elif fam == "pfb_synthesis" and a["bins"] != a["m"] and not (a["m"] % 2 == 0 and a["bins"] == a["m"] // 2 + 1):
            bad.append("bins neither M nor M / 2 + 1")
        if a["hop"] == 0:
            bad.append("D == 0")
        if fam == "pfb_analysis":
            if a["nx"] == 0:
                bad.append("nx == 0")
            if a["lead"] >= a["nh"]:
                bad.append("lead >= nh")
            if a["rows"] > 1 and a["row_stride"] < a["nx"]:
                bad.append("row_stride < nx")
        elif a["hop"] and a["out_first"] + a["out_len"] > (a["frames"] - 1) * a["hop"] + a["nh"]:
            bad.append("window past the full result")
    return bad


def within_caps(case: Case) -> bool:
    g, fam = case.g, case.family
    if fam in ("split32", "split64"):
        return g["batch"] * g["n"] <= SPLIT_MAX
    if fam == "czt":
        return g["batch"] * g["n"] * g["m"] <= CZT_MAX
    if fam == "goertzel":
        return g["batch"] * g["n"] * g["nfreq"] <= GOERTZEL_MAX
    if fam == "dht":
        return g["n"] <= DHT_MAX_N and g["batch"] * g["n"] <= DHT_MAX
    nx = g["row_stride"] if fam == "pfb_analysis" else synthesis_full(g)
    return g["rows"] * g["frames"] * g["m"] <= PFB_MAX and g["rows"] * nx <= PFB_MAX


# ---- the inputs of a case ---------------------------------------------------------------------------------------------------------------
def _data(rng, shape, specials, dtype=F):
    """uniform [-1, 1); with `specials` a few rows get special values (the three row kinds of test_gpu_rowwise_fuzz.py)"""
    x = rng.uniform(-1, 1, shape).astype(dtype)
    if specials and x.size:
        b, n = shape
        sp = SPECIALS.astype(dtype)
        for r in rng.choice(b, size=min(b, 1 + int(rng.integers(0, 4))), replace=False):
            kind = int(rng.integers(0, 3))
            if kind == 0:    # a whole row of one special value
                x[r] = rng.choice(sp)
            elif kind == 1:  # a few specials in a uniform row
                pos = rng.choice(n, size=min(n, 1 + int(rng.integers(0, 3))), replace=False)
                x[r, pos] = rng.choice(sp, size=pos.size)
            else:            # a row of specials
                x[r] = rng.choice(sp, size=n)
    return x


def inputs(case: Case) -> dict:
    rng = np.random.default_rng(case.data_seed)
    g, fam = case.g, case.family
    if fam in ("split32", "split64"):
        shape = (g["batch"], g["n"])
        return dict(re=_data(rng, shape, case.specials, case.real), im=_data(rng, shape, case.specials, case.real))
    if fam in ("czt", "dht"):
        return dict(x=_data(rng, (g["batch"], g["n"]), case.specials))
    if fam == "goertzel":
        return dict(x=_data(rng, (g["batch"], g["n"]), case.specials), freqs=goertzel_freqs(g))
    if fam == "pfb_analysis":
        return dict(x=_data(rng, (g["rows"], g["nx"]), case.specials), h=rng.uniform(-1, 1, g["nh"]).astype(F))
    rows, frames, bins = g["rows"], g["frames"], g["bins"]
    flat = _data(rng, (rows * frames, 2 * bins), case.specials)
    return dict(x=np.ascontiguousarray(flat).view(np.complex64).reshape(rows, frames, bins), h=rng.uniform(-1, 1, g["nh"]).astype(F))


def strided(x: np.ndarray, stride: int) -> np.ndarray:
    """The rows as the analysis sees them: (rows - 1) * stride + nx floats, NaN in the gaps."""
    rows, nx = x.shape
    flat = np.full((rows - 1) * stride + nx, np.nan, F)
    for r in range(rows):
        flat[r * stride:r * stride + nx] = x[r]
    return flat


def nan_safe(case: Case) -> bool:
    """NaNs in the same places count as equal whatever their sign (rowcheck): the special-value cases, and the chirp-Z sets that
    overflow or underflow on their own (an Inf - Inf is the platform's default NaN)."""
    return case.specials or (case.family == "czt" and case.g["set"] not in CZT_FINITE)


# ---- expected values: each family's existing oracle -----------------------------------------------------------------------------------
def expected(case: Case, inp: dict) -> dict:
    """name -> array of every output of the (valid) call.  The CPU oracle (oracle.pyoracle) must be built: split and the filter bank run
    their transforms on it."""
    g, fam = case.g, case.family
    with np.errstate(all="ignore"):
        if fam in ("split32", "split64"):
            from split_oracle import split_ref

            re, im = split_ref(inp["re"], inp["im"], bool(g["inverse"]))
            return dict(re=re, im=im)
        if fam == "czt":
            import spectral_oracle as so

            wr, wi, ar, ai = czt_params(g)
            return dict(out=so.czt(inp["x"], g["m"], (wr, wi), (ar, ai)).reshape(g["batch"], g["m"]))
        if fam == "goertzel":
            import spectral_oracle as so

            return dict(out=so.goertzel(inp["x"], g["rate"], inp["freqs"]).reshape(g["batch"], g["nfreq"]))
        if fam == "dht":
            import hartley_oracle as ho

            return dict(out=ho.dht(inp["x"]))
        import pfb_oracle as po

        if fam == "pfb_analysis":
            return dict(out=po.analysis_ref(inp["x"], inp["h"], g["m"], g["hop"], g["lead"], g["frames"], g["bins"]))
        full = po.synthesis_ref(inp["x"], inp["h"], g["m"], g["hop"], g["scale"])
        return dict(out=np.ascontiguousarray(full[:, g["out_first"]:g["out_first"] + g["out_len"]]))


# ---- float64 ----------------------------------------------------------------------------------------------------------------------------
FLOAT64_MIN_VALUES = 8   # framed_expected.CONV_FLOAT64_MIN_VALUES: a window of fewer values has no meaningful relative error
CZT_FLOAT64_MAX = 256    # the largest n and m at which test_spectral_cpu.py measured its bound (see float64_error)
CZT_BINS_CHECKED = 48
CZT_ROWS_CHECKED = 2


def _part_rel(got64, want_full64, part, count, full):
    """filter_cases._window_rel's measure: the L2 norm of the part's difference over the L2 norm of the whole float64 result scaled to
    the part's share of the values; None for fewer than FLOAT64_MIN_VALUES values of a longer result."""
    if count < min(FLOAT64_MIN_VALUES, full):
        return None
    den = float(np.linalg.norm(want_full64)) * np.sqrt(count / full)
    diff = float(np.linalg.norm(got64 - want_full64[part]))
    return diff / den if den else diff


def czt_float64(x, m, params, bins):
    """sum_i x[i] a^-i w^(i k) in float64 from the f32 w and a at the bins `bins`, and sum_i |term| (test_spectral_cpu._f64_czt's sums)"""
    wr, wi, ar, ai = params
    w64, a64 = complex(wr, wi), complex(ar, ai)
    n = x.shape[1]
    i = np.arange(n)[:, None]
    k = np.asarray(bins)[None, :]
    ainv = 0j if a64 == 0 else 1.0 / a64
    with np.errstate(all="ignore"):
        core = np.power(ainv, i) * np.power(w64, i * k) if n else np.zeros((0, k.size), complex)
    if a64 == 0 and n:
        core[0, :] = 1.0  # 0^0: apow starts at (1, 0)
    terms = x.astype(np.float64)[:, :, None] * core[None, :, :]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def analysis_float64(x, h, m, hop, lead, frames):
    """Z[k] = sum_{i < nh} h[i] x[f D + i - lead] exp(-2 pi i k i / M), all M bins, in float64: the products folded onto M points (the
    exponential has period M in i) and numpy's float64 transform"""
    rows, nx = x.shape
    nh = h.size
    xp = np.zeros((rows, lead + max(nx, frames * hop + nh)))
    xp[:, lead:lead + nx] = x
    seg = np.stack([xp[:, f * hop:f * hop + nh] for f in range(frames)], axis=1) * h.astype(np.float64)
    return np.fft.fft(seg.reshape(rows, frames, nh // m, m).sum(axis=2), axis=-1)


def float64_error(case: Case, inp: dict, out: dict, bounds: dict):
    """(error, bound) of a finite case's output against float64, in the measure and with the bound of the family's CPU test, which the
    caller hands in: bounds["czt"] = 4 * test_spectral_cpu.MEASURED_WORST, the factor of n * eps32 * sum |term| that
    test_czt_oracle_agrees_with_float64 asserts, here on the finite parameter sets, up to CZT_ROWS_CHECKED rows and CZT_BINS_CHECKED bins
    of a case with n, m <= 256, the sizes that test measured it at (w^k is w multiplied k times into (1, 0) and then raised to the
    i-th power the same way, both in f32, so the reference's own error grows like i * k * eps32, not like the n * eps32 of the bound:
    the oracle at n = 63, m = 4096 is at 7.5 times the factor, and bit for bit what the reference computes); bounds["pfb"] = test_pfb_cpu.bound(M, T, direction), relative L2, a window or a prefix of bins measured as
    filter_cases measures a window.  None: nothing to hold -- a family whose CPU test has no float64 bound (split, goertzel, dht: their
    oracles are held bit for bit to a second restatement instead), a chirp-Z set that leaves the finite range, an M = 6 bank (no
    bound exists for that Bluestein length), a window of a few values."""
    g, fam = case.g, case.family
    if fam == "czt":
        if g["set"] not in CZT_FINITE or g["n"] == 0 or max(g["n"], g["m"]) > CZT_FLOAT64_MAX:
            return None
        m = g["m"]
        rng = np.random.default_rng(case.data_seed + 1)
        bins = np.unique(np.concatenate([[0, m - 1], rng.integers(0, m, CZT_BINS_CHECKED)]))
        rows = sorted({0, g["batch"] - 1})[:CZT_ROWS_CHECKED]
        want, mag = czt_float64(inp["x"][rows], m, czt_params(g), bins)
        err = np.abs(np.asarray(out["out"])[rows][:, bins].astype(np.complex128) - want)
        eps = float(np.finfo(F).eps)
        return float(np.max(err / (g["n"] * eps * mag + 1e-300))), bounds["czt"]
    if fam not in ("pfb_analysis", "pfb_synthesis"):
        return None
    m, taps = g["m"], g["nh"] // g["m"]
    try:
        bound = bounds["pfb"](m, taps, 0 if fam == "pfb_analysis" else 1)
    except KeyError:
        return None
    got = np.asarray(out["out"])
    if fam == "pfb_analysis":
        want = analysis_float64(inp["x"], inp["h"], m, g["hop"], g["lead"], g["frames"])
        err = _part_rel(got.astype(np.complex128), want, (Ellipsis, slice(0, g["bins"])), g["bins"], m)
    else:
        want = bounds["synthesis_f64"](inp["x"], inp["h"], m, g["hop"], g["scale"])
        part = (Ellipsis, slice(g["out_first"], g["out_first"] + g["out_len"]))
        err = _part_rel(got.astype(np.float64), want, part, g["out_len"], want.shape[-1])
    return None if err is None else (err, bound)
