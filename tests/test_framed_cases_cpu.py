"""The draw of the frame-geometry fuzz (tests/framed_cases.py) and its expected values (tests/framed_expected.py) without a GPU: the
chunk formulas on hand-worked shapes, the coverage of the 16 seeds, the share of refused calls, the shared oracle pass against the
per-family oracles, and the oracle's one-sided frames against numpy.fft.rfft in float64.

Float64 bound.  The relative L2 error of a one-sided frame of the CPU oracle (whose bytes are the device's) against rfft of the
float64 windowed, zero-padded frame, the largest over up to 8 (row, frame) pairs of every finite case of the 16 seeds, per win_len
(framed_expected.MEASURED; every window length of the draw has a figure).  The bound is 2.5 x the measured maximum, the margin
of tests/test_convolve_cpu.py and of test_gpu_rowwise_fuzz.py's _float64_check: the reference's twiddle recurrence is deterministic per
n, so the error of a length varies little with the data.

    win_len   measured     win_len   measured     win_len   measured     win_len   measured
          1   4.22e-08          16   6.98e-08         128   6.39e-07        1024   1.51e-05
          2   4.92e-08          31   2.00e-06         256   5.69e-07        2048   7.92e-06
          3   2.22e-07          32   4.52e-07         400   4.67e-05        4096   9.40e-05
          5   2.52e-07          33   2.92e-06         512   1.08e-05        8192   4.82e-05
         15   1.60e-06          64   3.35e-07        1000   7.73e-05

Cost of expected() with the float64 check, per seed 0 .. 15 on one CPU core, seconds: 0.9 1.6 1.0 0.6 1.6 0.6 0.5 0.7 0.7 0.6 0.3 1.4 0.6
0.9 0.8 0.8 (the convolution rows included)."""
import time

import numpy as np
import pytest

import framed_cases as fc
import framed_expected as fe
import frontend_oracle as fo
import welch_oracle as wo

F = np.float32

@pytest.fixture(scope="module")
def drawn():
    return {seed: fc.cases(seed) for seed in range(fc.SEEDS)}


def test_the_draw_is_deterministic_and_within_the_caps(drawn):
    for seed, cs in drawn.items():
        again = fc.cases(seed)
        assert [c.describe() for c in cs] == [c.describe() for c in again]
        assert sum(c.kind == "framed" for c in cs) == 8 and sum(c.kind == "convolve" for c in cs) == 3
        assert sum(c.kind == "framed" and c.release_after >= 0 for c in cs) == 1 and sum(c.kind == "framed" and c.stream_at >= 0 for c in cs) == 1
        for c in cs:
            if c.kind == "convolve":
                assert c.block >= c.nh >= 1 and c.nx >= 1 and c.out_len >= 1 and c.out_first + c.out_len <= c.full, c.describe()
                assert c.rows * fc.ceil_div(c.full, c.hop) * c.block <= fc.CONV_MAX_POINTS, c.describe()
                continue
            assert c.win_len in fc.WINS and c.hop >= 1 and c.row_stride >= c.len and c.rows >= 1
            for fam, frames in c.frames.items():
                assert frames >= 1 and c.rows * frames * c.win_len <= fc.MAX_POINTS and c.rows * frames <= fc.MAX_FRAMES, (c.describe(), fam)
            if "picture" in c.frames:
                assert c.rows * c.frames["picture"] * (c.win_len // 2) <= fc.MAX_PIXELS, c.describe()
            assert sorted(fc.family_order(c)) == sorted(c.frames)
    streamed = {}
    for seed, cs in drawn.items():
        fams = [fc.stream_family(c) for c in cs if c.kind == "framed" and fc.stream_family(c) is not None]
        assert len(fams) == 1, f"seed {seed}: exactly one family call on the side stream, got {fams}"
        assert all(fc.refusal(c, fc.stream_family(c)) is None for c in cs if c.kind == "framed" and fc.stream_family(c)), f"seed {seed}: a refused call"
        streamed[fams[0]] = streamed.get(fams[0], 0) + 1
    print(f"families on the side stream: {streamed}")
    assert set(streamed) == set(fc.FRAME_FAMILIES), sorted(set(fc.FRAME_FAMILIES) - set(streamed))
    wins = {c.win_len for cs in drawn.values() for c in cs if c.kind == "framed"}
    assert wins == set(fc.WINS), sorted(set(fc.WINS) - wins)
    assert set(fe.MEASURED) == set(fc.WINS), "a float64 figure for every window length"


def test_chunk_formulas_on_known_shapes():
    """Each formula beside the figures the family's own seam test states (test_gpu_picture.py::test_chunk_seams_inside_a_row,
    welch_seams_child.py's shapes are of the same form)."""
    cap = fc.CHUNK_1MB
    # picture, win 1024, 3 x 601 frames: 2 KiB of magnitudes per frame, 512 per chunk; 256 under the running maximum
    assert fc.picture_chunk(1024, False, cap, 1803) == (1 << 20) // (4 * 512) == 512
    assert fc.picture_chunk(1024, True, cap, 1803) == (1 << 20) // (8 * 512) == 256
    assert [divmod(t, 601) for t in range(512, 1803, 512)] == [(0, 512), (1, 423), (2, 334)]
    # a Bluestein length keeps its composed frames too: 4 * 200 + 8 * 400 bytes
    assert fc.picture_chunk(400, False, cap, 10000) == (1 << 20) // 4000 == 262
    assert fc.frontend_chunk(400, cap, 10000) == 262 and fc.frontend_chunk(256, cap, 10000) == (1 << 20) // 512 == 2048
    assert fc.frontend_chunk(1, cap, 77) == 77                      # no bins: no bytes per frame, one chunk
    assert fc.composed_stft_chunk(256, cap, 5000) == 0 and fc.composed_stft_chunk(1000, cap, 5000) == (1 << 20) // 8000 == 131
    assert fc.chunk_rows(cap, 1 << 21, 5) == 1 and fc.chunk_rows(cap, 8, 5) == 5 and fc.chunk_rows(cap, 8, 0) == 0
    # Welch, win 256: 8 * 129 bytes of spectrum and ceil(4 * 129 / 32) = 17 of partial per frame: 999 frames, cut back to a group seam
    assert fc.welch_composed_cap(256, False, cap, 5000) == (1 << 20) // (8 * 129 + 17) == 999
    assert fc.welch_composed_cap(256, True, cap, 5000) == (1 << 20) // (16 * 129 + 33) == 500
    assert fc.welch_chunk_end(0, 999, 1100, 3300) == 992 and fc.welch_chunk_end(992, 999, 1100, 3300) == 1100 + 864
    assert fc.welch_chunk_end(0, 999, 500, 1500) == 500 + 480       # the seam of row 1's group 15
    assert fc.welch_chunk_end(0, 32, 40, 80) == 32 and fc.welch_chunk_end(32, 32, 40, 80) == 40   # a short last group goes alone
    assert fc.welch_chunk_end(0, 1000, 10, 30) == 30
    assert fc.welch_frames_walked(1000, 100, 50) == 10 and fc.welch_frames_walked(1001, 100, 50) == 11 and fc.welch_frames_walked(0, 7, 9) == 1
    # a walk by welch_chunk_end visits group seams only and covers the batch
    for frames, rows, c in ((1100, 3, 999), (70, 9, 100), (33, 40, 32), (5, 7, 32)):
        t, total = 0, frames * rows
        while t < total:
            e = fc.welch_chunk_end(t, c, frames, total)
            assert t < e <= total and ((e % frames) % fc.GROUP == 0 or e % frames == 0 or e == total)
            assert e - t <= max(c, fc.GROUP)
            t = e


def _count(drawn):
    counts, per_case = {}, []
    for cs in drawn.values():
        for c in cs:
            k = fc.classify(c)
            per_case.append((c, k))
            for name in k:
                counts[name] = counts.get(name, 0) + 1
    return counts, per_case


# every class classify can name
FRAMED_CLASSES = (["welch:fused", "welch:composed", "welch:small-n", "frontend:fused", "frontend:composed", "frontend:small-n", "mfcc:fused",
                   "mfcc:composed", "mfcc:in-frontend", "ctx:default", "ctx:chunk1", "hop<win", "hop==win", "hop>win", "len<win", "frames>required",
                   "welch_frames<required", "welch_frames>required", "last_group_short", "last_group_of_one", "one_group", "many_groups",
                   "stride_gap", "rows>1", "seam_inside_row", "seam_at_row_boundary", "no_seam", "seam_off_group", "bluestein", "odd_win",
                   "small_win", "specials", "caller_window", "picture:max_mode0", "picture:max_mode1", "picture:max_mode2", "refusal"]
                  + [f"form:{f}" for f in fc.FORMS])
CONV_CLASSES = (["conv:fused", "conv:composed", "conv:small-n", "conv_per_row", "conv_correlate", "conv_hop1", "conv_one_block", "conv_many_blocks",
                 "conv_starts_inside_a_block", "conv_ends_inside_a_block", "conv_chunk_seam"]
                + [f"conv_window:{w}" for w in ("full", "same", "valid", "inside", "last")] + [f"conv_form:{f}" for f in fc.FORMS])


def test_coverage_of_the_sixteen_seeds(drawn):
    counts, per_case = _count(drawn)
    for name in sorted(counts):
        print(f"{name}: {counts[name]}")
    assert set(counts) <= set(FRAMED_CLASSES + CONV_CLASSES), sorted(set(counts) - set(FRAMED_CLASSES + CONV_CLASSES))
    few = {name: counts.get(name, 0) for name in FRAMED_CLASSES + CONV_CLASSES if counts.get(name, 0) < 3}
    assert not few, f"classes in fewer than 3 cases: {few}"

    framed = [(c, k) for c, k in per_case if c.kind == "framed"]

    def own_seam(c, fams, inside):
        s = fc.seams(c)
        return any((t % fc.seam_frames(c, fam) != 0) == inside for fam in fams if fam in s for t in s[fam])

    pairs = {
        "seam_inside_row with fused Welch": [c for c, k in framed if {"seam_inside_row", "welch:fused"} <= k],
        "a composed Welch seam inside a row": [c for c, k in framed if "welch:composed" in k and own_seam(c, ("welch", "csd"), True)],
        "a running-maximum picture seam on a row boundary": [c for c, k in framed if "picture:max_mode1" in k and own_seam(c, ("picture",), False)],
        "hop>win with stride_gap": [c for c, k in framed if {"hop>win", "stride_gap"} <= k],
        "len<win with frames>required": [c for c, k in framed if {"len<win", "frames>required"} <= k],
        "bluestein on chunk1": [c for c, k in framed if {"bluestein", "ctx:chunk1"} <= k],
        "front end fused with 128 filters": [c for c, k in framed if "frontend:fused" in k and c.num_mel == 128],
        "front end composed with 129 filters": [c for c, k in framed if "frontend:composed" in k and c.num_mel == 129],
        "a last group of one frame below required": [c for c, k in framed if {"last_group_of_one", "welch_frames<required"} <= k],
    }
    for name, hit in pairs.items():
        print(f"{name}: {[(c.seed, c.index) for c in hit]}")
    missing = [name for name, hit in pairs.items() if not hit]
    assert not missing, missing
    chunk1 = [c for c, _ in framed if c.ctx == "chunk1"]
    over = [c for c in chunk1 if any(fc.seams(c).values())]
    print(f"chunk1 cases: {len(chunk1)}, with a family whose scratch exceeds 1 MiB: {len(over)}")
    assert 2 * len(over) >= len(chunk1)


def test_refused_calls_are_a_small_share(drawn):
    calls = refused = 0
    for cs in drawn.values():
        for c in cs:
            if c.kind != "framed":
                calls += 1
                continue
            for fam in c.frames:
                calls += 1
                refused += fc.refusal(c, fam) is not None
    print(f"refused family calls: {refused} of {calls} ({100.0 * refused / calls:.1f} %)")
    assert 0 < refused <= calls // 10


@pytest.mark.parametrize("seed", [0, 1])
def test_the_shared_pass_agrees_with_the_family_oracles(oracle, drawn, seed):
    """The one-sided prefix is welch_oracle.frames_of; the magnitudes are frontend_oracle.magnitudes (its oracle.stft_magnitudes path
    included); the Welch sums are welch_oracle.welch_ref's."""
    for c in drawn[seed]:
        if c.kind != "framed":
            continue
        inp = fc.inputs(c)
        exp = fe.expected(oracle, c, inp)
        win = exp["window"]
        K = c.win_len // 2 + 1
        with np.errstate(all="ignore"):
            for fam in ("onesided", "welch"):
                frames = c.frames[fam]
                for r in range(min(c.rows, 3)):
                    want = wo.frames_of(inp["x"][r], win, c.hop, frames)
                    assert exp["S"][r, :frames, :K].tobytes() == want.tobytes(), (c.describe(), fam, r)
            for fam in ("mags", "mel", "picture"):
                if fam not in c.frames or c.frames[fam] < c.required:
                    continue
                frames = c.frames[fam]
                want = fo.magnitudes(oracle, inp["x"], c.win_len, c.hop, frames, inp["window"])
                got = fe.magnitudes_of(exp["S"][:, :frames], c.win_len)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c.describe(), fam)
            if c.rows * c.frames["welch"] <= 2000:
                want = wo.welch_ref(inp["x"], win, c.hop, c.frames["welch"], c.welch_scale, c.welch_double)
                assert exp["welch"].tobytes() == want.tobytes(), c.describe()
                want = wo.welch_ref(inp["x"], win, c.hop, c.frames["csd"], c.welch_scale, c.welch_double, y=inp["y"])
                assert exp["csd"].tobytes() == want.tobytes(), c.describe()


def test_float64_check_of_the_oracle(oracle, drawn):
    """Every finite case of the 16 seeds: the one-sided frames against rfft in float64 within 2.5 x the measured maximum of their
    win_len; the convolution rows against numpy in float64 within test_convolve_cpu.py's bound.  Prints the maxima and the time of
    expected() per seed."""
    worst, conv_worst, conv_cut_worst, times = {}, {}, {}, []
    for seed, cs in drawn.items():
        t0 = time.perf_counter()
        for c in cs:
            if c.kind == "convolve":
                inp = fc.conv_inputs(c)
                from convolve_oracle import convolve_ref

                full = convolve_ref(inp["x"], inp["h"], c.block, c.correlate).astype(np.float64)
                err = fe.conv_float64_error(c, inp, full)
                conv_worst[c.block] = max(conv_worst.get(c.block, 0.0), err)
                assert err <= fe.conv_float64_bound(c.block), (c.describe(), err)
                cut = fe.conv_float64_error(c, inp, full[:, c.out_first:c.out_first + c.out_len], c.out_first)  # the window the device is held to
                assert (cut is None) == (c.out_len < min(fe.CONV_FLOAT64_MIN_VALUES, c.full)), c.describe()
                if cut is not None:
                    conv_cut_worst[c.block] = max(conv_cut_worst.get(c.block, 0.0), cut)
                    assert cut <= fe.conv_float64_bound(c.block), (c.describe(), cut)
                continue
            inp = fc.inputs(c)
            exp = fe.expected(oracle, c, inp)
            if c.specials or not isinstance(exp.get("onesided"), np.ndarray):
                continue
            for err in fe.float64_errors(c, inp, exp["window"], exp["onesided"]):
                worst[c.win_len] = max(worst.get(c.win_len, 0.0), err)
                bound = fe.float64_bound(c.win_len)
                assert bound is not None and err <= bound, (c.describe(), err, bound)
        times.append(time.perf_counter() - t0)
    print("float64, one-sided frames: " + ", ".join(f"{w}: {worst[w]:.3g}" for w in sorted(worst)))
    print("float64, convolve: " + ", ".join(f"{b}: {conv_worst[b]:.3g}" for b in sorted(conv_worst)))
    print("float64, convolve windows: " + ", ".join(f"{b}: {conv_cut_worst[b]:.3g}" for b in sorted(conv_cut_worst)))
    print("expected() and its float64 check per seed, seconds: " + " ".join(f"{t:.1f}" for t in times))
