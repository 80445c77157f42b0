"""Deterministic cases of the robust M-estimator solve (IMLS_SOLVE_ROBUST), shared by
test_robust_cases.py — which proves on the CPU restatement alone (robust_np.py) that each case does
what it is meant to — and test_gpu_robust.py, which runs them on the device.  No GPU imports.

The device changes its code path at two places (csrc/solve_robust.hip): float rows of ≤ 4096
(kSmallRows) take one block, each thread holding rows t + k·512; every other frame, and every fp64
row set, takes the grid chain of 256-row slabs.  The sizes below sit on both sides of those edges.
"""
import functools
import pathlib

import numpy as np

from planetary_lidar_odometry_amd import _abi, config
from ransac_cases import config_a_pair, hdl_strided, outlier_set

POSE_TOL = 1e-6                          # the project's bound for every LS-family solve
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
LOSSES = ("huber", "cauchy", "geman_mcclure")
SCALES = (0.1, 0.5)
ITERATIONS = (1, 5, 32)
ROW_SIZES = (1, 5, 6, 255, 256, 257, 4096, 4097, 16385, 40000)        # fp64 rows: 256-row slabs, kSmallRows
PROJECT_SIZES = (6, 64, 511, 512, 513, 4095, 4096, 4097)              # float rows: rows per thread, the switch
TRUE_X = np.array([0.0, 0.0, 0.02, 0.3, -0.1, 0.05])                   # the motion of outlier_set()
BRANCH_SHARE = 0.02                      # at least this share of the rows on each side of |r| = c


def robust_params(loss="huber", scale=0.1, iterations=5, iters=10):
    """The shipped config with the Robust loop method."""
    p = config.params_from_config(config.load())
    p.solve_method = _abi.IMLS_SOLVE_ROBUST
    p.robust_loss = config.ROBUST_LOSS[loss]
    p.robust_scale = scale
    p.robust_iterations = iterations
    p.iterations = iters
    return p


def golden(name):
    return dict(np.load(GOLDEN / f"{name}.npz"))


def caller_weights(n, seed=11):
    return np.random.default_rng(seed).uniform(0.2, 1.0, n)


def below_scale_set(n=500, seed=3):
    """Rows of a small motion with 1 mm noise: every |r| stays far below c = 0.5 at every iterate
    (|b| ≤ ~0.15), so every Huber weight is 1 and the solve is unit-weight LS."""
    rng = np.random.default_rng(seed)
    s = rng.uniform(-3, 3, (n, 3))
    nrm = rng.normal(0, 1, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = 0.005
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    d = s @ R.T + np.array([0.03, -0.02, 0.01]) + nrm * rng.normal(0, 0.001, (n, 1))
    return s, d, nrm


# ---- float rows through project() + solve(): three orthogonal plane patches ---------------------------
PLANE_SPACING = 0.2


@functools.lru_cache(maxsize=None)
def planes_map():
    """(M, 6) float32: z = 0, x = 0 and y = 0 patches over [1, 7]² on a 0.2 m grid with their normals.
    The patches are ≥ 1 m apart, so a query's 20 nearest neighbours lie on its own patch."""
    g = np.arange(1.0, 7.0 + 1e-9, PLANE_SPACING)
    u, v = (m.ravel() for m in np.meshgrid(g, g, indexing="ij"))
    z = np.zeros_like(u)
    parts = []
    for axis in range(3):
        pts = np.stack([z, u, v], 1)
        pts = np.roll(pts, axis, axis=1)            # axis 0: x = 0; 1: y = 0; 2: z = 0
        nrm = np.zeros_like(pts)
        nrm[:, axis] = 1.0
        parts.append(np.concatenate([pts, nrm], 1))
    return np.concatenate(parts).astype(np.float32)


def planes_source(n, seed=5):
    """(n, 6) float32 near the patches' interiors ([2, 6]²): a small rigid motion away, 2 cm noise
    along the normal and a quarter of the points 0.15 … 0.3 m off their plane (|r| > 0.1)."""
    rng = np.random.default_rng(seed + n)
    axis = np.arange(n) % 3
    uv = rng.uniform(2.0, 6.0, (n, 2))
    off = rng.normal(0, 0.02, n)
    far = rng.random(n) < 0.25
    off[far] = rng.uniform(0.15, 0.3, far.sum()) * rng.choice([-1.0, 1.0], far.sum())
    pts = np.zeros((n, 3))
    nrm = np.zeros((n, 3))
    for k in range(3):
        m = axis == k
        p = np.stack([off[m], uv[m, 0], uv[m, 1]], 1)
        pts[m] = np.roll(p, k, axis=1)
        nrm[m, k] = 1.0
    a = 0.004
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    pts = (pts - 4.0) @ R.T + 4.0 + np.array([0.02, -0.015, 0.01])
    return np.concatenate([pts, nrm @ R.T], 1).astype(np.float32)


# ---- registrations ----------------------------------------------------------------------------------
# name -> (builder of (source rows, target rows), scale c, the range n_valid must lie in at every iteration)
def _golden_pair(name):
    g = golden(name)
    return np.ascontiguousarray(g["src"].T), np.ascontiguousarray(g["tgt"].T)


FRAMES = {
    "vlp16_pair": (lambda: _golden_pair("vlp16_pair"), 0.1, (6, 4097)),
    "planetary_pair": (lambda: _golden_pair("planetary_pair"), 0.02, (6, 4097)),
    "config-a": (config_a_pair, 0.1, (4097, 16385)),
    "hdl-stride5": (lambda: hdl_strided(5), 0.1, (16385, 1 << 30)),
}
FRAME_ITERS = 3


def rows6(cloud):
    """(N, 6) float32 x y z nx ny nz of a PointXYZINormal array or an (N, 6) array."""
    import model_restatement as mr
    return mr.xyzn(cloud)
