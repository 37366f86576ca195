"""The draw of the spectral fuzz (tests/spectral_cases.py) without a GPU: determinism, caps and preconditions (every
valid case passes every check of its header block in the library itself, called with a null context; the one refused case of a seed
gets its code), the coverage of the 16 seeds -- every family x route x form, every class and every kind of refusal --, the state the
draw leaves on each context (chirp-Z keys through a 4-slot LRU, Goertzel coefficient sets, Hartley lengths), the chunk formulas on
hand-worked shapes, the oracles against each other on drawn cases, and the float64 bounds the GPU test applies, held here by the
float32 oracles' own output on every finite drawn case.

Float64 bounds, each the one of the family's CPU test:
  czt            |out - float64 sum| <= 4 * MEASURED_WORST * n * eps32 * sum |term| per bin (test_spectral_cpu.py:
                 test_czt_oracle_agrees_with_float64), the finite parameter sets, 2 rows and up to 50 bins of a case
  pfb_analysis   relative L2 <= test_pfb_cpu.bound(M, T, 0), a prefix of bins measured as filter_cases measures a window
  pfb_synthesis  relative L2 <= test_pfb_cpu.bound(M, T, 1) against test_pfb_cpu.synthesis_f64, a window measured the same way
  split, goertzel, dht   their CPU tests (test_split_cpu.py, test_spectral_cpu.py, test_hartley_cpu.py) hold no float64 bound -- each
                 holds its oracle bit for bit to a second restatement -- and none is invented here: the same is done on drawn cases
                 (test_the_oracles_agree_with_each_other_on_drawn_cases)
The chirp-Z factor holds at n, m <= 256, the sizes test_spectral_cpu.py measured it at, and is applied there only
(spectral_cases.float64_error says why it does not extend).  Measured on the oracles, the worst error / bound of a family over the 16
seeds: czt 0.087, pfb_analysis 0.16, pfb_synthesis 0.11.

Cost of expected() with its float64 check, per seed 0 .. 15 on one CPU core, seconds: 0.1 0.3 0.2 0.2 0.1 0.3 0.0 0.2 0.0 0.6 0.3 0.1 0.1
0.0 0.3 0.0 (it bounds the host time of the GPU test, which computes the same values)."""
import time

import numpy as np
import pytest

import spectral_cases as sc

F = np.float32


@pytest.fixture(scope="module")
def drawn():
    return {seed: sc.cases(seed) for seed in range(sc.SEEDS)}


def float64_bounds():
    """name -> the bound of the family's CPU test (see the module docstring)"""
    from test_pfb_cpu import bound as pfb_bound
    from test_pfb_cpu import synthesis_f64
    from test_spectral_cpu import MEASURED_WORST

    return {"czt": 4 * MEASURED_WORST, "pfb": pfb_bound, "synthesis_f64": synthesis_f64}


def _valid(drawn):
    return [c for cs in drawn.values() for c in cs if c.refuse is None]


def test_the_draw_is_deterministic_and_within_the_caps(drawn):
    for seed, cs in drawn.items():
        again = sc.cases(seed)
        assert [c.describe() for c in cs] == [c.describe() for c in again]
        assert [(c.release_before, c.side_stream, c.data_seed) for c in cs] == [(c.release_before, c.side_stream, c.data_seed) for c in again]
        assert len(cs) == sc.PER_SEED and [c.index for c in cs] == list(range(sc.PER_SEED))
        assert sum(c.refuse is not None for c in cs) == 1, f"seed {seed}: exactly one refused call"
        assert sum(c.release_before for c in cs) == 1 and not cs[0].release_before, f"seed {seed}: one release between two cases"
        assert all(c.refuse is None for c in cs if c.release_before or c.side_stream), f"seed {seed}: the release and the side stream go with valid cases"
        assert sum(c.side_stream for c in cs) == 1, f"seed {seed}: one valid case on a side stream"
        assert [(c.family, c.route, c.form) for c in cs if c.refuse is None] == [sc._combo(seed * sc.VALID_PER_SEED + k) for k in range(sc.VALID_PER_SEED)]
        for c in cs:
            assert c.form in sc.FORMS[c.family] and c.route in sc.ROUTES[c.family] and c.ctx in ("default", "chunk1"), c.describe()
            broken = sc.header_violations(c)
            if c.refuse is None:
                assert sc.within_caps(c), c.describe()
                assert not broken, (c.describe(), broken)
            else:
                assert len(broken) == 1, (c.describe(), broken)  # (two would leave the code to the order of the header's checks)
    streamed = {c.family for c in _valid(drawn) if c.side_stream}
    assert streamed == set(sc.FAMILIES), sorted(set(sc.FAMILIES) - streamed)
    kinds = [(c.family, c.refuse["what"]) for cs in drawn.values() for c in cs if c.refuse]
    assert sorted(kinds) == sorted(sc.REFUSALS) and len(set(kinds)) == 16
    refused = {fam if not fam.startswith("split") else "split" for fam, _ in kinds}
    assert refused == {"split", "czt", "goertzel", "dht", "pfb_analysis", "pfb_synthesis"}


def test_the_library_accepts_every_valid_case_and_refuses_the_others(drawn, hiplib):
    """Both entry points of every case with a null context: every check of the header block comes before the context is looked at, so
    a valid call gets as far as KOFFT_ERR_NULL and the refused one returns its code.  No device is touched.  Two kinds of refusal lie
    behind the null check and need a context: overlapping device buffers (the header puts that check last) and the setter's unknown
    route; with a null context they too must get as far as KOFFT_ERR_NULL, and tests/test_gpu_spectral_fuzz.py sees their codes."""
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    ptrs = dict(x=p, h=p, out=p, re=p, im=p, re_out=p, im_out=p, freqs=p)
    late = 0
    for cs in drawn.values():
        for c in cs:
            behind_null = bool(c.refuse and (c.refuse.get("overlap") or c.refuse.get("setter")))
            late += behind_null
            for host, stem in ((True, "kofft_hip_"), (False, "kofft_hip_dev_")):
                rc = sc.invoke(getattr(hiplib, stem + sc.ENTRY[c.family]), None, c, ptrs, host)
                assert rc == (c.refuse["code"] if c.refuse and not behind_null else sc.NULL), (c.describe(), stem, rc)
            if c.refuse and c.refuse.get("setter"):
                name, value = c.refuse["setter"]
                assert getattr(hiplib, name)(None, value) == sc.NULL
    assert late == 3
    assert not buf.any()


# every class classify can name beside family x route x form; each must be hit at least twice
CLASSES = ["specials", "release_before", "side_stream", "ctx:default", "ctx:chunk1",
           "split:fused", "split:composed", "split:inverse", "split:forward", "split:fused_range_end_or_neighbour", "split:just_past_the_fused_range",
           "split:composed_only_n", "split:n1", "split:bluestein", "split:batch_at_rows_per_chunk", "split:chunk_seam",
           "czt:set_dft", "czt:set_zoom", "czt:set_spiral", "czt:set_a_zero", "czt:set_grow", "czt:set_dft_a0", "czt:n0", "czt:m_at_256", "czt:longest",
           "czt:batch_at_rows_per_block", "czt:batch_at_64", "czt:key_that_comes_back", "czt:key_dht_length", "czt:direct_tiled0", "czt:direct_tiled1",
           "goertzel:vector_loads", "goertzel:scalar_loads", "goertzel:n%4==0", "goertzel:n%4!=0", "goertzel:nfreq_at_256", "goertzel:one_frequency",
           "goertzel:most_frequencies", "goertzel:batch_at_rows_per_block", "goertzel:coeff_first", "goertzel:coeff_repeat", "goertzel:coeff_prefix",
           "goertzel:coeff_again",
           "dht:tiled_kernel", "dht:simple_kernel", "dht:table_on_device", "dht:table_on_host", "dht:batch_at_64", "dht:n_at_256", "dht:tiny_n",
           "dht:longest", "dht:n%4!=0",
           "analysis:fused", "analysis:composed", "synthesis:fused", "synthesis:composed", "pfb:composed_only_m", "pfb:fused_range_end", "pfb:bluestein",
           "pfb:m1", "pfb:taps1", "pfb:taps2", "pfb:taps3", "pfb:taps8", "pfb:hop_gt_nh", "pfb:hop_gt_m", "pfb:hop_m", "pfb:hop_lt_m", "pfb:hop1",
           "pfb:items_at_workgroup_multiple", "pfb:many_workgroups", "pfb:rows>1",
           "analysis:off_alignment_composed", "analysis:measured_choice_composed", "analysis:lead_0", "analysis:lead_nh-1", "analysis:lead_nh-hop",
           "analysis:frames_past_the_end", "analysis:stride_gap", "analysis:bins_1", "analysis:bins_m", "analysis:bins_one_sided",
           "analysis:chunk_seam", "analysis:items_at_chunk",
           "synthesis:bins_m", "synthesis:bins_one_sided", "synthesis:scale_1", "synthesis:scale_other", "synthesis:window_whole",
           "synthesis:window_inside", "synthesis:window_one", "synthesis:window_last", "synthesis:window_skip_chunks", "synthesis:chunk_seam",
           "synthesis:seam_inside_a_row", "synthesis:composed:chunk_shorter_than_back", "synthesis:composed:back_clamped",
           "synthesis:composed:hop_gt_nh_across_a_seam", "synthesis:fused:chunk_shorter_than_back", "synthesis:fused:back_clamped",
           "synthesis:fused:hop_gt_nh_across_a_seam", "synthesis:seam_window_and_hop_gt_nh", "synthesis:chunk_left_out"]
ONCE = ["refusal"] + [f"refusal:{fam}:{what}" for fam, what in sc.REFUSALS]   # (one refusal of every kind; "refusal" itself 16 times)
COMBO_CLASSES = [f"{fam}:route{r}:{form}" for fam in sc.FAMILIES for r in sc.ROUTES[fam] for form in sc.FORMS[fam]]
OTHER = [f"family:{fam}" for fam in sc.FAMILIES] + [f"refusal:{fam}" for fam in sc.FAMILIES] + ["pfb:taps_other", "analysis:lead_other"]


def test_coverage_of_the_sixteen_seeds(drawn):
    counts = {}
    valid = 0
    for cs in drawn.values():
        for c in cs:
            valid += c.refuse is None
            for name in sc.classify(c):
                if c.refuse is None or name not in COMBO_CLASSES:  # (a refused call runs nothing: it counts for no family x route x form)
                    counts[name] = counts.get(name, 0) + 1
    for name in sorted(counts):
        print(f"{name}: {counts[name]}")
    assert valid == sc.VALID and len(sc.COMBOS) == 60 and set(sc.COMBOS) == {(f, r, fo) for f in sc.FAMILIES for r in sc.ROUTES[f] for fo in sc.FORMS[f]}
    known = set(CLASSES + COMBO_CLASSES + OTHER + ONCE)
    assert set(counts) <= known, sorted(set(counts) - known)
    few = {name: counts.get(name, 0) for name in CLASSES + COMBO_CLASSES if counts.get(name, 0) < 2}
    assert not few, f"classes in fewer than 2 cases: {few}"
    assert all(counts.get(name, 0) >= 1 for name in ONCE) and counts["refusal"] == sc.SEEDS


def test_the_state_the_draw_leaves_on_each_context(drawn):
    """The sequence of the 16 seeds in order, per context, as the library keeps its state (k_spectral_f32.hip, k_hartley_f32.hip).
    Chirp-Z: a 4-slot LRU by (n, m, w, a), every route takes a slot, n == 0 none, release_scratch empties it -- at least six distinct
    keys per context, and at least two uses per context of a key that was there before and has been evicted since.  Goertzel: the
    device forms keep the last coefficient set -- per context a call with the bits of the call before (nothing uploaded), then a
    shorter prefix of them, then the whole set again.  Hartley: a length of a dht case is also the n of a table-route chirp-Z case of
    the same context (route 2, or route 0 at a batch from which it takes the table), at least twice per context."""
    import spectral_oracle as so

    for ctx in ("default", "chunk1"):
        slots, seen, evicted, tables = [], set(), set(), set()
        back = 0
        last, events = None, []
        dht_n, czt_n = set(), set()
        for seed in range(sc.SEEDS):
            for c in drawn[seed]:
                if c.ctx != ctx or c.refuse or c.family == "split64":  # (split64 runs on the f64 pair of contexts)
                    continue
                if c.release_before:
                    evicted.clear()  # (dropped, not evicted: a rebuild after a release is the context test's)
                    slots, last = [], None
                    tables.clear()
                if c.family == "czt":
                    key = sc.czt_key(c.g)
                    if key is None:
                        continue
                    if key in slots:
                        slots.remove(key)
                    elif key in evicted:
                        back += 1
                        evicted.discard(key)
                    slots.insert(0, key)
                    seen.add(key)
                    if len(slots) > sc.CZT_SLOTS:
                        evicted.add(slots.pop())
                        tables.intersection_update(slots)
                    # czt_use_table: route 0 takes the table from batch 2 where it is there, from batch 8 where it is not
                    if c.route == 2 or (c.route == 0 and c.g["batch"] >= (2 if key in tables else 8)):
                        tables.add(key)
                        czt_n.add(c.g["n"])
                elif c.family == "goertzel" and c.form != "host":
                    bits = so.goertzel_coeff(c.g["n"], c.g["rate"], sc.goertzel_freqs(c.g)).tobytes()
                    if last is None:
                        events.append("upload")
                    elif bits == last:
                        events.append("same")
                    elif len(bits) < len(last) and last.startswith(bits):
                        events.append("prefix")
                    else:
                        events.append("upload")
                    last = bits
                elif c.family == "dht":
                    dht_n.add(c.g["n"])
        print(f"{ctx}: {len(seen)} chirp-Z keys, {back} came back after their eviction; goertzel device calls: {' '.join(events)}; "
              f"dht lengths also on the chirp-Z table route: {sorted(dht_n & czt_n)}")
        assert len(seen) >= 6 and back >= 2, (ctx, len(seen), back)
        assert any(events[i:i + 3] == ["same", "prefix", "upload"] for i in range(len(events))), (ctx, events)
        assert len(dht_n & czt_n) >= 2, (ctx, sorted(dht_n), sorted(czt_n))


def _case(family, route, form, ctx, **g):
    return sc.Case(0, 0, family, route, form, ctx, False, 0, g)


def test_the_chunk_formulas_on_hand_worked_shapes():
    """scratch_chunk_rows for the three chunked routes and the synthesis walk with its `back`, against numbers worked by hand."""
    assert sc.chunk_rows(1 << 20, 8000, 200) == 131 and sc.chunk_rows(1 << 20, 8000, 100) == 100 and sc.chunk_rows(1 << 20, 1 << 21, 3) == 1
    assert sc.chunk_rows(1 << 20, 0, 7) == 7 and sc.chunk_rows(1 << 20, 8, 0) == 0
    # split: 1 MiB / (1000 * 8) = 131 rows of c32, 65 of c64
    assert sc.split_chunk(_case("split32", 0, "dev_oop", "chunk1", n=1000, batch=132)) == 131
    assert sc.split_chunk(_case("split64", 0, "dev_oop", "chunk1", n=1000, batch=132)) == 65
    assert sc.split_chunk(_case("split32", 0, "dev_oop", "default", n=1000, batch=132)) == 132
    assert sc.split_fused(_case("split32", 1, "host", "default", n=1 << 14, batch=1)) and not sc.split_fused(_case("split64", 1, "host", "default", n=1 << 14, batch=1))
    assert not sc.split_fused(_case("split32", 0, "host", "default", n=64, batch=1)) and not sc.split_fused(_case("split32", 1, "host", "default", n=1, batch=1))
    # analysis, composed: 1 MiB / (240 * 8) = 546 items
    assert sc.analysis_chunk(_case("pfb_analysis", 0, "dev", "chunk1", m=240, rows=3, frames=200)) == 546
    # the fused routes: the measured choice stops the analysis at M = 1024, the switch at 2 does not; x off 4-byte alignment: composed
    assert sc.pfb_fused(_case("pfb_analysis", 1, "dev", "default", m=1024)) and not sc.pfb_fused(_case("pfb_analysis", 1, "dev", "default", m=2048))
    assert sc.pfb_fused(_case("pfb_analysis", 2, "dev", "default", m=4096)) and not sc.pfb_fused(_case("pfb_analysis", 2, "dev_unaligned", "default", m=64))
    assert sc.pfb_fused(_case("pfb_synthesis", 1, "dev", "default", m=4096)) and not sc.pfb_fused(_case("pfb_synthesis", 1, "dev", "default", m=8192))
    assert not sc.pfb_fused(_case("pfb_synthesis", 2, "dev", "default", m=16)) and not sc.pfb_fused(_case("pfb_synthesis", 0, "dev", "default", m=64))
    # synthesis: the issue's example -- M = 65536, T = 2, D = M / 4, 12 frames: 1 MiB / (65536 * 8) = 2 frames a chunk, back = 8 - 1 = 7
    a = _case("pfb_synthesis", 0, "dev", "chunk1", m=65536, nh=131072, hop=16384, rows=1, frames=12, out_first=0, out_len=11 * 16384 + 131072)
    assert sc.synthesis_chunk(a) == 2 and sc.synthesis_back(a.g) == 7 and sc.synthesis_full(a.g) == 311296
    assert sc.synthesis_walk(a) == [(0, 2, 0, True), (2, 2, 2, True), (4, 2, 4, True), (6, 2, 6, True), (8, 2, 7, True), (10, 2, 7, True)]
    # two rows of 10 frames, 8 a chunk, back = 15 clamped to 9: the chunks start at frame 8 of row 0 and frame 6 of row 1
    b = _case("pfb_synthesis", 0, "dev", "chunk1", m=16384, nh=131072, hop=8192, rows=2, frames=10, out_first=0, out_len=9 * 8192 + 131072)
    assert sc.synthesis_back(b.g) == 15 and sc.synthesis_walk(b) == [(0, 8, 0, True), (8, 8, 8, True), (16, 4, 6, True)]
    # the fused inverse keeps M floats a frame: 64 frames a chunk at M = 4096; D = 96 under 8192 taps: back = 86 - 1
    f = _case("pfb_synthesis", 1, "dev", "chunk1", m=4096, nh=8192, hop=96, rows=1, frames=130, out_first=0, out_len=129 * 96 + 8192)
    assert sc.synthesis_chunk(f) == 64 and sc.synthesis_back(f.g) == 85 and [w[2] for w in sc.synthesis_walk(f)] == [0, 64, 85]
    # a window behind the first chunk's samples [0, 128 * 1): the first chunk runs nothing; one inside them: the last does not
    w = _case("pfb_synthesis", 0, "dev", "chunk1", m=1024, nh=3072, hop=1, rows=1, frames=200, out_first=128, out_len=50)
    assert sc.synthesis_walk(w) == [(0, 128, 0, False), (128, 72, 128, True)]
    w.g.update(out_first=5, out_len=100)
    assert sc.synthesis_walk(w) == [(0, 128, 0, True), (128, 72, 128, False)]
    # D > nh: frame f owns [f D, (f + 1) D), the gap included; the default context has one chunk
    assert sc.synthesis_walk(_case("pfb_synthesis", 0, "dev", "default", m=16, nh=16, hop=21, rows=3, frames=4, out_first=0, out_len=79)) == [(0, 12, 0, True)]


def test_refused_calls_are_one_in_ten(drawn):
    calls = sum(len(cs) for cs in drawn.values())
    refused = sum(c.refuse is not None for cs in drawn.values() for c in cs)
    assert 0 < refused <= calls // 10


def test_the_oracles_agree_with_each_other_on_drawn_cases(oracle, drawn):
    """split_ref is the oracle's interleaved transform; the analysis with T = 1 and lead = 0 is the oracle's STFT with window h and hop
    D; the vectorised czt is czt_scalar on a sample of bins (the DFT parameters on the case's n and m) and the vectorised goertzel is
    goertzel_scalar on a sample of (row, frequency); dht over the cached table is dht over a table of the sampled columns alone."""
    import hartley_oracle as ho
    import pfb_oracle as po
    import spectral_oracle as so
    from split_oracle import split_ref

    seen = {"split": 0, "stft": 0, "czt": 0, "goertzel": 0, "dht": 0}
    with np.errstate(all="ignore"):
        for c in _valid(drawn):
            g = c.g
            rng = np.random.default_rng(c.data_seed + 2)
            if c.family in ("split32", "split64") and g["batch"] <= 5:
                inp = sc.inputs(c)
                z = np.empty(inp["re"].shape, np.complex64 if c.family == "split32" else np.complex128)
                z.real, z.imag = inp["re"], inp["im"]
                want = oracle.fft(z, bool(g["inverse"]))
                re, im = split_ref(inp["re"], inp["im"], bool(g["inverse"]))
                assert re.tobytes() == np.ascontiguousarray(want.real).tobytes() and im.tobytes() == np.ascontiguousarray(want.imag).tobytes(), c.describe()
                seen["split"] += 1
            elif c.family == "pfb_analysis" and g["m"] > 1 and g["rows"] * g["nx"] <= 1 << 16 and g["nx"] // g["hop"] <= 4096:
                inp = sc.inputs(c)
                m, hop, nx = g["m"], g["hop"], g["nx"]
                h = np.ascontiguousarray(inp["h"][:m])
                frames = -(-nx // hop)
                got = po.analysis_ref(inp["x"], h, m, hop, 0, frames, m)
                for r in range(g["rows"]):
                    assert got[r].tobytes() == oracle.stft_mt(inp["x"][r], h, hop, frames).reshape(frames, m).tobytes(), (c.describe(), r)
                seen["stft"] += 1
            elif c.family == "czt" and 1 <= g["n"] <= 1024:
                x = sc.inputs(c)["x"][:1]
                n, m = g["n"], g["m"]
                w, a = so.param_sets(m)["dft"]
                full = so.czt(x, m, w, a)[0]
                hi = min(m, 24)   # (czt_scalar multiplies w into (1, 0) k times for bin k and walks the row once per bin)
                bins = sorted({0, hi - 1, *rng.integers(0, hi, 3).tolist()})
                assert so.czt_scalar(x[0], hi, w, a)[bins].tobytes() == full[bins].tobytes(), c.describe()
                seen["czt"] += 1
            elif c.family == "goertzel" and g["n"] <= 1024:
                inp = sc.inputs(c)
                full = so.goertzel(inp["x"], g["rate"], inp["freqs"]).reshape(g["batch"], g["nfreq"])
                for _ in range(3):
                    r, j = int(rng.integers(0, g["batch"])), int(rng.integers(0, g["nfreq"]))
                    one = so.goertzel_scalar(inp["x"][r], g["rate"], inp["freqs"][j])
                    assert np.array([one], F).tobytes() == full[r, j:j + 1].tobytes() or (np.isnan(one) and np.isnan(full[r, j])), (c.describe(), r, j)
                seen["goertzel"] += 1
            elif c.family == "dht" and g["n"] >= 2:
                x = sc.inputs(c)["x"][:2]
                cols = ho.sample_cols(g["n"], 8, c.data_seed)
                assert ho.dht(x, cols=cols).tobytes() == np.ascontiguousarray(ho.dht(x)[:, cols]).tobytes(), c.describe()
                seen["dht"] += 1
    print(seen)
    assert min(seen.values()) >= 5, seen


def test_float64_bounds_hold_for_the_oracles_on_every_finite_case(oracle, drawn):
    """The check the GPU test applies to the device's output, applied to the oracle's: every finite valid case of the 16 seeds.  Prints
    the worst error / bound per family and the time of expected() and the check per seed."""
    bounds = float64_bounds()
    worst, times = {}, []
    for seed, cs in drawn.items():
        t0 = time.perf_counter()
        for c in cs:
            if c.refuse:
                continue
            inp = sc.inputs(c)
            exp = sc.expected(c, inp)
            if c.specials:
                continue
            res = sc.float64_error(c, inp, exp, bounds)
            if res is None:
                continue
            err, bound = res
            worst[c.family] = max(worst.get(c.family, 0.0), err / bound)
            assert err <= bound, f"{c.describe()}: float64 error {err:.3g} > {bound:.3g}"
        times.append(time.perf_counter() - t0)
    print("worst error / bound: " + ", ".join(f"{k}: {v:.2g}" for k, v in sorted(worst.items())))
    print("expected() and its float64 check per seed, seconds: " + " ".join(f"{t:.1f}" for t in times))
    assert set(worst) == {"czt", "pfb_analysis", "pfb_synthesis"}
