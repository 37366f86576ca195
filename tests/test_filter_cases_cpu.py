"""The draw of the filter and lapped fuzz (tests/filter_cases.py) without a GPU: determinism, caps and preconditions
(every valid case passes every check of its header block in the library itself, called with a null context; the one refused case of a
seed gets its code), the coverage of the 16 seeds, the oracles against each other on drawn cases, and the float64 bounds the GPU test
applies, held here by the float32 oracles' own output on every finite drawn case.

Float64 bounds, each the one of the family's CPU test:
  resample       |out - float64 sum| <= resample_oracle.forward_bound per output (test_resample_cpu.py), up to 4 rows of a case
  sosfilt        max|y - scipy float64| / max|scipy float64| <= 2 * FILTFILT_MEASURED = 4.4e-5 (test_sosfilt_cpu.py's one float64 bound)
  sosfilt_scan   the same measure <= 2 * FILTFILT_SCAN_MEASURED = 5.02e-5 (test_sosfilt_scan_cpu.py's bound for the cascades of
                 sosfilt_oracle.designs() at chunks 64 and 1024; its per-design table belongs to poles within 1e-3 of the unit circle, and
                 the cascades drawn here keep theirs at radius 0.5 .. 0.9 as sosfilt_oracle.cascade does)
  convolve_bank  relative L2 <= 1e-6 + 2e-7 * block (test_convolve_bank_cpu.py), a window measured as framed_expected.conv_float64_error
                 measures it
  dct4 / mdct / imdct   relative L2 <= test_mdct_cpu.bound(N), an IMDCT window measured the same way
Measured on the oracles, the worst error / bound of a family over the 16 seeds: resample 0.42, sosfilt 0.033, sosfilt_scan 0.032,
convolve_bank 0.35, dct4 0.09, imdct 0.11, mdct 0.48.

Cost of expected() with its float64 check, per seed 0 .. 15 on one CPU core, seconds: 0.4 0.1 0.1 0.6 0.1 0.6 0.5 0.5 0.2 0.2 0.3 0.2 0.3
0.5 0.4 0.2 (it bounds the host time of the GPU test, which computes the same values)."""
import ctypes as C
import time

import numpy as np
import pytest

import filter_cases as fc

F = np.float32


@pytest.fixture(scope="module")
def helpers(hiplib):
    return fc.Helpers.from_lib(hiplib)


@pytest.fixture(scope="module")
def drawn(helpers):
    return {seed: fc.cases(seed, helpers) for seed in range(fc.SEEDS)}


def float64_bounds():
    """family -> the bound of its CPU test (see the module docstring)"""
    import resample_oracle as ro
    from test_convolve_bank_cpu import _bound as bank_bound
    from test_mdct_cpu import bound as dct_bound
    from test_sosfilt_cpu import FILTFILT_MEASURED
    from test_sosfilt_scan_cpu import FILTFILT_SCAN_MEASURED

    return {"resample": ro.forward_bound, "sosfilt": 2 * FILTFILT_MEASURED, "sosfilt_scan": 2 * FILTFILT_SCAN_MEASURED,
            "convolve_bank": bank_bound, "dct": dct_bound}


def test_the_draw_is_deterministic_and_within_the_caps(drawn, helpers):
    for seed, cs in drawn.items():
        again = fc.cases(seed, helpers)
        assert [c.describe() for c in cs] == [c.describe() for c in again]
        assert [(c.release_before, c.side_stream) for c in cs] == [(c.release_before, c.side_stream) for c in again]
        assert len(cs) == fc.PER_SEED and [c.index for c in cs] == list(range(fc.PER_SEED))
        assert sum(c.refuse is not None for c in cs) == 1, f"seed {seed}: exactly one refused call"
        assert sum(c.release_before for c in cs) == 1 and not cs[0].release_before, f"seed {seed}: one release between two cases"
        assert sum(c.side_stream for c in cs) == 1 and all(c.refuse is None for c in cs if c.side_stream), f"seed {seed}: one valid case on a side stream"
        for c in cs:
            assert c.form in fc.FORMS[c.family] and c.route in fc.ROUTES[c.family] and c.ctx in ("default", "chunk1"), c.describe()
            broken = fc.header_violations(c)
            if c.refuse is None:
                assert fc.within_caps(c), c.describe()
                assert not broken, (c.describe(), broken)
            else:
                assert broken, c.describe()
    streamed = {c.family for cs in drawn.values() for c in cs if c.side_stream}
    assert streamed == set(fc.FAMILIES), sorted(set(fc.FAMILIES) - streamed)
    refused = {c.family for cs in drawn.values() for c in cs if c.refuse}
    assert refused == set(fc.FAMILIES), sorted(set(fc.FAMILIES) - refused)


def test_the_library_accepts_every_valid_case_and_refuses_the_others(drawn, hiplib):
    """Both entry points of every case with a null context: every check of the header block comes before the context is looked at, so
    a valid call gets as far as KOFFT_ERR_NULL and the refused one returns its code.  No device is touched."""
    buf = np.zeros(64, F)
    p = buf.ctypes.data
    ptrs = dict(x=p, h=p, sos=p, out=p, window=p, zi=None, zf=None)
    for cs in drawn.values():
        for c in cs:
            for stem in ("kofft_hip_", "kofft_hip_dev_"):
                rc = fc.invoke(getattr(hiplib, stem + fc.ENTRY[c.family]), None, c, ptrs)
                assert rc == (c.refuse["code"] if c.refuse else fc.NULL), (c.describe(), stem, rc)
    assert not buf.any()


# every class classify can name beside family x route x form; each must be hit at least twice
CLASSES = ["specials", "refusal", "release_before", "side_stream", "ctx:default", "ctx:chunk1",
           "resample:route_flip", "resample:kernel_tiled", "resample:kernel_plain", "resample:nh_at_up", "resample:one_tap", "resample:not_coprime",
           "resample:tile_edge", "resample:one_output", "resample:rows_at_256", "resample:t0_zero", "resample:t0_centre", "resample:t0_random",
           "resample:full_length",
           "sosfilt:group_edge", "sosfilt:many_passes", "sosfilt:zi", "sosfilt:no_zi", "sosfilt:zf", "sosfilt:no_zf", "sosfilt:reverse", "sosfilt:forward",
           "sosfilt:route_edge_16_rows", "sosfilt:wave_edge_64_rows", "sosfilt:tile_edge", "sosfilt:tiny_row", "sosfilt:kernel_tiled", "sosfilt:kernel_plain",
           "sosfilt_scan:group_edge", "sosfilt_scan:many_passes", "sosfilt_scan:zi", "sosfilt_scan:no_zi", "sosfilt_scan:zf", "sosfilt_scan:no_zf",
           "sosfilt_scan:reverse", "sosfilt_scan:forward", "sosfilt_scan:chunk32", "sosfilt_scan:chunk64", "sosfilt_scan:chunk96", "sosfilt_scan:chunk1024",
           "sosfilt_scan:64_chunk_edge", "sosfilt_scan:nx_at_chunk_multiple", "sosfilt_scan:one_chunk", "sosfilt_scan:pieces_of_rows", "sosfilt_scan:rows_at_64",
           "bank:fused", "bank:composed", "bank:small", "bank:fused_range_neighbour", "bank:fused_range_end", "bank:off_alignment_composed",
           "bank:complex_taps", "bank:real_taps", "bank:correlate", "bank:out_real", "bank:out_complex", "bank:out_magnitude", "bank:window_full",
           "bank:window_same", "bank:window_valid", "bank:window_inside", "bank:filters1", "bank:filters2", "bank:filters5", "bank:hop1", "bank:one_block",
           "bank:many_blocks", "bank:chunk_seam",
           "dct:fused", "dct:composed", "dct:composed_only_n", "dct:bluestein", "dct:off_alignment_composed", "dct:items_at_workgroup_multiple",
           "dct:many_workgroups", "dct:chunk_seam", "dct4:fused", "dct4:composed", "mdct:fused", "mdct:composed", "imdct:fused", "imdct:composed",
           "mdct:lead_0", "mdct:lead_n", "mdct:lead_other", "mdct:frames_past_the_end", "mdct:stride_gap", "mdct:rows>1",
           "imdct:window_whole", "imdct:window_from_n", "imdct:window_random", "imdct:scale_2/n", "imdct:scale_other", "imdct:one_frame", "imdct:chunk_seam"]
COMBO_CLASSES = [f"{fam}:route{r}:{form}" for fam in fc.FAMILIES for r in fc.ROUTES[fam] for form in fc.FORMS[fam]]
OTHER = [f"family:{fam}" for fam in fc.FAMILIES] + [f"refusal:{fam}" for fam in fc.FAMILIES]


def test_coverage_of_the_sixteen_seeds(drawn, helpers):
    counts = {}
    valid = 0
    for cs in drawn.values():
        for c in cs:
            valid += c.refuse is None
            for name in fc.classify(c, helpers):
                if c.refuse is None or name not in COMBO_CLASSES:  # (a refused call runs nothing: it counts for no family x route x form)
                    counts[name] = counts.get(name, 0) + 1
    for name in sorted(counts):
        print(f"{name}: {counts[name]}")
    assert valid == fc.SEEDS * fc.VALID_PER_SEED
    known = set(CLASSES + COMBO_CLASSES + OTHER)
    assert set(counts) <= known, sorted(set(counts) - known)
    few = {name: counts.get(name, 0) for name in CLASSES + COMBO_CLASSES if counts.get(name, 0) < 2}
    assert not few, f"classes in fewer than 2 cases: {few}"


def test_refused_calls_are_one_in_ten(drawn):
    calls = sum(len(cs) for cs in drawn.values())
    refused = sum(c.refuse is not None for cs in drawn.values() for c in cs)
    assert 0 < refused <= calls // 10


def test_the_oracles_agree_with_each_other_on_drawn_cases(oracle, drawn):
    """sosfilt_scan_ref with one chunk is sosfilt_ref; convolve_bank_ref with real taps and the real kind is convolve_ref per filter;
    imdct_ref(mdct_ref(x)) with a sine window, lead = N and scale = 2 / N gives x back within test_mdct_cpu.ROUND_TRIP; resample_ref lies
    within forward_bound of the float64 sum (the float64 test below, which runs every finite resample case)."""
    import mdct_oracle as mo
    from convolve_bank_oracle import convolve_bank_ref
    from convolve_oracle import convolve_ref
    from sosfilt_oracle import sosfilt_ref
    from sosfilt_scan_oracle import sosfilt_scan_ref
    from test_mdct_cpu import ROUND_TRIP, rel

    seen = {"scan": 0, "bank": 0, "mdct": 0}
    with np.errstate(all="ignore"):
        for cs in drawn.values():
            for c in cs:
                if c.refuse:
                    continue
                g = c.g
                if c.family in ("sosfilt", "sosfilt_scan") and g["rows"] <= 65:
                    inp = fc.inputs(c)
                    one = -(-g["nx"] // fc.T) * fc.T  # one chunk over the whole row
                    a = sosfilt_scan_ref(inp["sos"], inp["x"], one, inp["zi"], g["reverse"])
                    b = sosfilt_ref(inp["sos"], inp["x"], inp["zi"], g["reverse"])
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), c.describe()
                    seen["scan"] += 1
                elif c.family == "convolve_bank" and not g["complex_taps"]:
                    inp = fc.inputs(c)
                    got = convolve_bank_ref(inp["x"], inp["h"], g["block"], g["correlate"], "real")
                    for f in range(g["filters"]):
                        assert got[:, f].tobytes() == convolve_ref(inp["x"], inp["h"][f], g["block"], g["correlate"]).tobytes(), (c.describe(), f)
                    seen["bank"] += 1
                elif c.family == "mdct" and g["n"] in ROUND_TRIP and not c.specials:
                    n = g["n"]
                    x = fc.inputs(c)["x"]
                    w = fc.sine_window(n)
                    frames = -(-g["nx"] // n) + 1
                    full = mo.imdct_ref(mo.mdct_ref(x, w, n, frames), w, 2.0 / n)
                    err = rel(full[:, n:n + g["nx"]], x)
                    assert err <= ROUND_TRIP[n], (c.describe(), err)
                    seen["mdct"] += 1
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
            inp = fc.inputs(c)
            exp = fc.expected(c, inp)
            if c.specials:
                continue
            res = fc.float64_error(c, inp, exp, bounds)
            if res is None:
                continue
            err, bound = res
            worst[c.family] = max(worst.get(c.family, 0.0), err / bound)
            assert err <= bound, f"{c.describe()}: float64 error {err:.3g} > {bound:.3g}"
        times.append(time.perf_counter() - t0)
    print("worst error / bound: " + ", ".join(f"{k}: {v:.2g}" for k, v in sorted(worst.items())))
    print("expected() and its float64 check per seed, seconds: " + " ".join(f"{t:.1f}" for t in times))
    assert set(worst) == set(fc.FAMILIES)
