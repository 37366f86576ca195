"""The definition of kofft_hip_sosfilt_scan_f32 (include/kofft_hip.h) in numpy float32, on top of
sosfilt_oracle.sosfilt_ref: per group of at most GROUP sections, with C = ceil(nx / chunk) chunks a row and D = 2 S state components,

  1. M[i][j]: component i of the state after walking ``chunk`` samples of +0 from the unit state e_j;
  2. p_c, c < C - 1: the state after walking chunk c from the +0 state;
  3. Z_0 = zi, Z_{c+1}[i] = ((((M[i][0] Z_c[0]) + (M[i][1] Z_c[1])) + ..) + (M[i][J-1] Z_c[J-1])) + p_c[i], J = 2 (i // 2) + 2;
  4. chunk c of the output is the walk of chunk c from Z_c, zf the state after chunk C - 1.

The walks run vectorised over "virtual rows" (every chunk of every row is a row of sosfilt_ref); the carry is a loop over the chunks in
float32 arrays, in the stated order of sums.  ``reverse`` is defined as flip, forward, flip."""
import numpy as np

from sosfilt_oracle import sosfilt_ref

F = np.float32
GROUP = 8  # KOFFT_HIP_SOSFILT_GROUP
TILE = 32  # KOFFT_HIP_SOSFILT_TILE


def transition(sos, chunk):
    """M [D, D] of one group: M[i, j] as step 1 says."""
    S = sos.shape[0]
    D = 2 * S
    _, cols = sosfilt_ref(sos, np.zeros((D, chunk), F), np.eye(D, dtype=F).reshape(D, S, 2))
    return np.ascontiguousarray(cols.reshape(D, D).T)  # cols[j] is column j


def carry(M, z0, p):
    """Z [rows, C, D] from Z_0 = z0 [rows, D] and p [rows, C - 1, D], step 3."""
    rows, seams, D = p.shape
    Z = np.empty((rows, seams + 1, D), F)
    Z[:, 0] = z0
    J = 2 * (np.arange(D) // 2) + 2
    with np.errstate(all="ignore"):
        for c in range(seams):
            zc = Z[:, c]
            acc = M[None, :, 0] * zc[:, 0:1]
            for j in range(1, D):
                acc = np.where(j < J, acc + (M[None, :, j] * zc[:, j:j + 1]), acc)
            Z[:, c + 1] = acc + p[:, c]
    assert Z.dtype == F
    return Z


def _group_forward(sos, v, chunk, z0):
    """One group over v [rows, nx] from z0 [rows, S, 2]: (y, zf)."""
    rows, nx = v.shape
    S = sos.shape[0]
    D = 2 * S
    C = (nx - 1) // chunk + 1
    if C == 1:
        return sosfilt_ref(sos, v, z0)
    full = (C - 1) * chunk
    _, p = sosfilt_ref(sos, v[:, :full].reshape(rows * (C - 1), chunk))
    Z = carry(transition(sos, chunk), z0.reshape(rows, D), p.reshape(rows, C - 1, D))
    out = np.empty_like(v)
    y, _ = sosfilt_ref(sos, v[:, :full].reshape(rows * (C - 1), chunk), Z[:, :C - 1].reshape(rows * (C - 1), S, 2))
    out[:, :full] = y.reshape(rows, full)
    out[:, full:], zf = sosfilt_ref(sos, v[:, full:], Z[:, C - 1].reshape(rows, S, 2))
    return out, zf


def sosfilt_scan_ref(sos, x, chunk, zi=None, reverse=False):
    """(y [rows, nx], zf [rows, sections, 2]) of x [rows, nx] (or one row [nx]: then y [nx], zf [sections, 2])."""
    sos = np.asarray(sos, F)
    x = np.asarray(x, F)
    assert chunk > 0 and chunk % TILE == 0
    one = x.ndim == 1
    v = np.array(x.reshape(-1, x.shape[-1]), F, copy=True)
    if reverse:
        v = np.ascontiguousarray(v[:, ::-1])
    rows = v.shape[0]
    sections = sos.shape[0]
    z = np.zeros((rows, sections, 2), F) if zi is None else np.array(np.asarray(zi, F).reshape(rows, sections, 2), copy=True)
    for g in range(0, sections, GROUP):
        v, z[:, g:g + GROUP] = _group_forward(sos[g:g + GROUP], v, chunk, z[:, g:g + GROUP].copy())
    if reverse:
        v = np.ascontiguousarray(v[:, ::-1])
    assert v.dtype == F and z.dtype == F
    return (v[0], z[0]) if one else (v, z)


def sosfiltfilt_scan_ref(sos, x, chunk, padlen=None):
    """kofft_amd.iir.sosfiltfilt(chunk=...): sosfilt_oracle.sosfiltfilt_ref with both passes through the scan."""
    from sosfilt_oracle import default_padlen, sosfilt_zi_ref

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
    y, _ = sosfilt_scan_ref(sos, ext, chunk, zi[None, :, :] * ext[:, :1, None])
    y, _ = sosfilt_scan_ref(sos, y, chunk, zi[None, :, :] * y[:, -1:, None], reverse=True)
    return np.ascontiguousarray(y[:, edge:edge + nx]).reshape(x.shape)
