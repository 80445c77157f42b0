"""Deterministic inputs of the pose-info tests, shared by test_pose_info_model.py (which proves on the
CPU what each case is meant to be) and test_gpu_pose_info.py (which runs them on the device).  No GPU
imports.

solve_rows(N):        N correspondences of a known small motion on three plane families, 5 mm of noise
                      along the normal (N = 1031: the golden x1 / y1 / n1 of vlp16_pair).
sentinel_rows(side):  the golden set with one row's target moved along its normal so that the row's
                      |r₁| sits just inside ("in": rank hi) or just outside ("out": rank hi + 1) the
                      upper trim boundary at ls_threshold 0.02.  Both sets keep hi − lo + 1 rows, but
                      the kept sets differ by that row: H differs by its a·aᵀ.
plane_rows():         the rows of test_gpu_ransac.py::test_drpm_degenerate_plane.
flat_rows():          300 rows on the plane z = 0 with normals exactly (0, 0, 1).
"""
import functools
import pathlib

import numpy as np

import pose_info_np as pin

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
SIZES = (6, 7, 63, 64, 65, 255, 256, 257, 1031, 4096, 4097)
THRESHOLDS = (0.0, 0.02, 0.25)
SENTINEL_T = 0.02
SENTINEL_ROW = 500


@functools.lru_cache(maxsize=None)
def golden(name):
    return dict(np.load(GOLDEN / f"{name}.npz"))


@functools.lru_cache(maxsize=None)
def solve_rows(N):
    if N == 1031:
        g = golden("vlp16_pair")
        return tuple(g[k].astype(np.float64) for k in ("x1", "y1", "n1"))
    rng = np.random.default_rng(100 + N)
    s = rng.uniform(-15, 15, (N, 3))
    nrm = np.zeros((N, 3))
    nrm[np.arange(N), np.arange(N) % 3] = 1.0
    nrm += rng.normal(0, 0.05, (N, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = 0.01
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    d = s @ R.T + np.array([0.2, -0.1, 0.05]) + nrm * rng.normal(0, 0.005, (N, 1))
    return s, d, nrm


@functools.lru_cache(maxsize=None)
def sentinel_rows(side):
    """(s, d, n) with row SENTINEL_ROW placed at rank hi ("in") or hi + 1 ("out") of the order (|r₁|, row)."""
    s, d, n = (v.copy() for v in solve_rows(1031))
    j = SENTINEL_ROW
    lo, hi = pin.trim_ranks(len(s), SENTINEL_T)
    others = np.arange(len(s)) != j
    nn = float(n[j] @ n[j])
    for _ in range(8):                    # b_j moves x0 a little: a few fixed-point rounds settle it
        a, b = pin.rows_ab(s, d, n)
        x0 = pin.solve_x(a, b)
        r1 = np.abs(pin.dot_seq(a, x0) - b)
        ro = np.sort(r1[others])
        # among the others, ranks hi − 1 | hi | hi + 1: the row goes between the first two ("in":
        # it takes rank hi) or between the last two ("out": it takes rank hi + 1)
        want = 0.5 * (ro[hi - 1] + ro[hi]) if side == "in" else 0.5 * (ro[hi] + ro[hi + 1])
        # residual a·x0 − b = −want  ⇔  b = a·x0 + want; b moves by δ when d moves by δ·n/‖n‖²
        delta = (float(pin.dot_seq(a[j:j + 1], x0)[0]) + want) - b[j]
        d[j] = d[j] + n[j] * (delta / nn)
    return s, d, n


@functools.lru_cache(maxsize=None)
def plane_rows():
    rng = np.random.default_rng(11)
    n_pts = 3000
    s = np.column_stack([rng.uniform(-10, 10, n_pts), rng.uniform(-10, 10, n_pts), rng.normal(0, 0.01, n_pts)])
    nrm = np.tile([0.0, 0.0, 1.0], (n_pts, 1)) + rng.normal(0, 0.02, (n_pts, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    d = s + np.array([0.2, 0.1, 0.05])
    return s, d, nrm


@functools.lru_cache(maxsize=None)
def flat_rows():
    rng = np.random.default_rng(3)
    s = np.column_stack([rng.uniform(-10, 10, 300), rng.uniform(-10, 10, 300), np.zeros(300)])
    nrm = np.tile([0.0, 0.0, 1.0], (300, 1))
    d = s + np.array([0.0, 0.0, 0.05]) + nrm * rng.normal(0, 0.01, (300, 1))
    return s, d, nrm
