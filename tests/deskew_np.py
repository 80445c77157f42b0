"""numpy restatement of imls_deskew (include/imls_gpu.h): per-point motion compensation
from the relative time the front end leaves in intensity = ring + scan_period·relTime
(scan_registration.cpp:1042-1048), as TransformToStart / TransformToEnd apply it
(laser_odometry.cpp:62-114).  Double arithmetic from the float inputs in the written order, each
coordinate rounded to float once.  The library differs from this only in its sin / cos (a few double
ulps), so a float result can differ by one ulp at the point's scale."""
import math

import numpy as np


def motion_parts(motion):
    """(a, θ, t, R) of a 4×4 motion (start ← end); ValueError where the library returns IMLS_ERR_ARG."""
    M = np.asarray(motion, dtype=np.float64).reshape(4, 4)
    if not np.isfinite(M).all():
        raise ValueError("non-finite motion entry")
    R, t = M[:3, :3], M[:3, 3]
    v = [0.5 * (R[2, 1] - R[1, 2]), 0.5 * (R[0, 2] - R[2, 0]), 0.5 * (R[1, 0] - R[0, 1])]
    nv = math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    theta = math.atan2(nv, (((R[0, 0] + R[1, 1]) + R[2, 2]) - 1.0) / 2.0)
    if not theta < math.pi / 2:
        raise ValueError("rotation of 90 degrees or more")
    a = [0.0, 0.0, 1.0] if nv == 0.0 else [v[0] / nv, v[1] / nv, v[2] / nv]
    return a, theta, t.copy(), R.copy()


def sweep_fraction(intensity, scan_period):
    """s = (I − float(int(I))) / scan_period with int as x86-64 truncates (INT_MIN out of range), the
    subtraction in float, the division in double; not clamped."""
    I = np.asarray(intensity, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        in_range = (I > np.float32(-2147483904.0)) & (I < np.float32(2147483648.0))
        whole = np.where(in_range, np.trunc(I), np.float32(-2147483648.0)).astype(np.float32)
        return (I - whole).astype(np.float64) / np.float64(np.float32(scan_period))


def _rodrigues(a, c, sn, p):
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    cx, cy, cz = a[1] * pz - a[2] * py, a[2] * px - a[0] * pz, a[0] * py - a[1] * px
    k = ((a[0] * px + a[1] * py) + a[2] * pz) * (1.0 - c)
    return np.stack([(px * c + cx * sn) + a[0] * k, (py * c + cy * sn) + a[1] * k, (pz * c + cz * sn) + a[2] * k], 1)


def _rt_mul(R, v):
    # Rᵀ·v, row by row, ((· + ·) + ·)
    return np.stack([(R[0, r] * v[:, 0] + R[1, r] * v[:, 1]) + R[2, r] * v[:, 2] for r in range(3)], 1)


def deskew_np(xyzi, motion, to="end", scan_period=0.1, normals=None):
    """The deskewed copy of xyzi ((n, 4+) float32: x, y, z, intensity, further columns kept) — with
    normals ((n, 3+) float32) the pair (xyzi, normals).  A row with a non-finite coordinate or
    intensity is kept bit for bit (its normal too), and so is a normal with a non-finite component;
    an identity motion returns the input's bytes."""
    if to not in ("end", "start"):
        raise ValueError("to: 'end' or 'start'")
    if not (np.isfinite(np.float32(scan_period)) and np.float32(scan_period) > 0):
        raise ValueError("scan_period must be positive")
    out = np.array(xyzi, dtype=np.float32, order="C")
    nout = None if normals is None else np.array(normals, dtype=np.float32, order="C")
    a, theta, t, R = motion_parts(motion)
    M = np.asarray(motion, dtype=np.float64).reshape(4, 4)
    if np.array_equal(M, np.eye(4)) or len(out) == 0:
        return out if nout is None else (out, nout)
    live = np.isfinite(out[:, :4]).all(axis=1)
    p = out[live, :3].astype(np.float64)
    s = sweep_fraction(out[live, 3], scan_period)
    phi = s * theta
    c, sn = np.cos(phi), np.sin(phi)
    q = _rodrigues(a, c, sn, p) + s[:, None] * t[None, :]
    if to == "end":
        q = _rt_mul(R, q - t[None, :])
    out[live, :3] = q.astype(np.float32)
    if nout is None:
        return out
    rows = np.nonzero(live)[0]
    fin = np.isfinite(nout[rows, :3]).all(axis=1)
    m = _rodrigues(a, c[fin], sn[fin], nout[rows[fin], :3].astype(np.float64))
    if to == "end":
        m = _rt_mul(R, m)
    nout[rows[fin], :3] = m.astype(np.float32)
    return out, nout
