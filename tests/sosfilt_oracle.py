"""The definition of kofft_hip_sosfilt_f32 (include/kofft_hip.h) in numpy float32, vectorised over rows, one sample
and one section at a time: per row, section s ascending, sample t ascending (descending with ``reverse``), with the section's input v
and state (z0, z1)

    y = (b0 * v) + z0;   z0 = ((b1 * v) - (a1 * y)) + z1;   z1 = (b2 * v) - (a2 * y)

every product and sum one float32 operation (numpy float32 arrays: no fusing, subnormals kept).  The state is [rows, sections, 2], the
layout of the C entry.  ``sosfiltfilt_ref`` is the composition kofft_amd.iir.sosfiltfilt documents, on top of sosfilt_ref."""
import numpy as np

F = np.float32


def sosfilt_ref(sos, x, zi=None, reverse=False):
    """(y [rows, nx], zf [rows, sections, 2]) of x [rows, nx] (or one row [nx]: then y [nx], zf [sections, 2])."""
    sos = np.asarray(sos, F)
    x = np.asarray(x, F)
    one = x.ndim == 1
    v = np.array(x.reshape(-1, x.shape[-1]), F, copy=True)
    rows, nx = v.shape
    sections = sos.shape[0]
    assert sos.shape == (sections, 6) and (sos[:, 3] == 1).all()
    z = np.zeros((rows, sections, 2), F) if zi is None else np.array(np.asarray(zi, F).reshape(rows, sections, 2), copy=True)
    order = range(nx - 1, -1, -1) if reverse else range(nx)
    with np.errstate(all="ignore"):
        for s in range(sections):
            b0, b1, b2, _, a1, a2 = sos[s]
            z0, z1 = z[:, s, 0].copy(), z[:, s, 1].copy()
            for t in order:
                xt = v[:, t]
                y = (b0 * xt) + z0
                z0 = ((b1 * xt) - (a1 * y)) + z1
                z1 = (b2 * xt) - (a2 * y)
                v[:, t] = y
            z[:, s, 0], z[:, s, 1] = z0, z1
    assert v.dtype == F and z.dtype == F
    return (v[0], z[0]) if one else (v, z)


def sosfilt_zi_ref(sos):
    """The closed form of the steady state of a unit step, float64 [sections, 2]."""
    sos = np.asarray(sos, np.float64)
    zi = np.empty((sos.shape[0], 2))
    scale = 1.0
    for s, (b0, b1, b2, _, a1, a2) in enumerate(sos):
        k = (b0 + b1 + b2) / (1.0 + a1 + a2)
        z1 = b2 - a2 * k
        zi[s] = scale * (b1 - a1 * k + z1), scale * z1
        scale = scale * k
    return zi


def default_padlen(sos):
    sos = np.asarray(sos)
    return 3 * (2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def sosfiltfilt_ref(sos, x, padlen=None):
    """Odd extension in float32, forward with state f32(zi) * ext[0], backward with state f32(zi) * y[last], the middle nx samples."""
    sos = np.asarray(sos, F)
    x = np.asarray(x, F)
    a = x.reshape(-1, x.shape[-1])
    nx = a.shape[1]
    edge = default_padlen(sos) if padlen is None else padlen
    assert nx > edge
    ext = a
    if edge:
        ext = np.concatenate([(F(2) * a[:, :1]) - a[:, edge:0:-1], a, (F(2) * a[:, -1:]) - a[:, -2:-(edge + 2):-1]], axis=1)
    zi = sosfilt_zi_ref(sos).astype(F)
    y, _ = sosfilt_ref(sos, ext, zi[None, :, :] * ext[:, :1, None])
    y, _ = sosfilt_ref(sos, y, zi[None, :, :] * y[:, -1:, None], reverse=True)
    return np.ascontiguousarray(y[:, edge:edge + nx]).reshape(x.shape)


def designs():
    """The cascades of the tests as float32 [sections, 6] arrays, by name: Butterworth 2, 4, 5, 6 and 8 (low, high, band) and an
    8th-order elliptic low-pass with poles close to the unit circle."""
    from scipy import signal

    out = {}
    for order in (2, 4, 5, 6, 8):
        out[f"butter{order}_low"] = signal.butter(order, 0.2, "low", output="sos")
        out[f"butter{order}_high"] = signal.butter(order, 0.3, "high", output="sos")
        out[f"butter{order}_band"] = signal.butter(order, [0.2, 0.5], "band", output="sos")
    out["ellip8"] = signal.ellip(8, 0.1, 80, 0.05, output="sos")
    return {k: np.ascontiguousarray(v, F) for k, v in out.items()}


def cascade(sections, seed=0):
    """A stable cascade of `sections` biquads for the shape ladders: poles of radius 0.5 .. 0.9 at seeded angles, seeded numerators."""
    rng = np.random.default_rng(29000 + seed + sections)
    r = rng.uniform(0.5, 0.9, sections)
    th = rng.uniform(0.2, 2.9, sections)
    sos = np.empty((sections, 6), F)
    sos[:, :3] = rng.uniform(-1, 1, (sections, 3))
    sos[:, 3] = 1
    sos[:, 4] = -2 * r * np.cos(th)
    sos[:, 5] = r * r
    return sos
