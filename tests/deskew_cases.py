"""Shared inputs of the deskew tests: noise-free moving VLP-16 sweeps with the world point of every
return, and the geometric bound a correct deskew has to meet."""
import functools
import math

import numpy as np

from planetary_lidar_odometry_amd import _abi, synth

# the per-sweep motion of the measurements in DESIGN §2d: 1 m and 3° per sweep
MOTION = synth.pose_xyyaw(1.0, 0.05, math.radians(3.0), 0.01, 0.002, 0.004)
POSE_START = synth.pose_xyyaw(12.0, -0.4, 0.3, 0.0, 0.003, -0.002)


def model(step_deg=0.8):
    """A noise-free 16-ring model: what the deskew leaves is then the front end's relTime alone."""
    return synth.ScanModel(np.arange(-15.0, 15.0 + 1e-9, 2.0), step_deg, 0.5, 100.0, range_noise=0.0, xyz_jitter=0.0)


def front_params():
    p = _abi.ImlsFrontParams()
    p.n_scans, p.minimum_range, p.maximum_range, p.scan_period, p.is_dense = 16, 0.5, 100.0, 0.1, 0
    return p


@functools.lru_cache(maxsize=None)
def moving_sweep(k=0, step_deg=0.8):
    """(raw (n, 3) float32, world hits (n, 3), true fractions (n,), pose at the sweep's start, motion)
    of sweep k of a platform that repeats MOTION every sweep."""
    pose = POSE_START
    for _ in range(k):
        pose = pose @ MOTION
    raw, hits, frac = synth.raw_sweep_moving(synth.make_scene(3), model(step_deg), pose, MOTION, 70 + k,
                                             start_deg=24.0 * k, return_hits=True)
    for a in (raw, hits, frac):
        a.setflags(write=False)
    return raw, hits, frac, pose, MOTION


def n_az(step_deg=0.8):
    return len(np.arange(0.0, 360.0, step_deg))


def geometry_bound(motion, xyz, step_deg=0.8):
    """(1/n_az + 2e-5)·(‖t‖ + θ·r_max) + 1e-4 metres.  1/n_az: the front end's relTime spans
    endOri − startOri over n_az − 1 firing steps; 2e-5: the float intensity's quantum (~1e-6) over
    scan_period; ‖t‖ + θ·r_max: the lever of a time error; 1e-4: float storage of the coordinates."""
    M = np.asarray(motion, dtype=np.float64)
    theta = math.acos(min(1.0, (np.trace(M[:3, :3]) - 1.0) / 2.0))
    r_max = float(np.linalg.norm(np.asarray(xyz, np.float64)[:, :3], axis=1).max())
    return (1.0 / n_az(step_deg) + 2e-5) * (float(np.linalg.norm(M[:3, 3])) + theta * r_max) + 1e-4


def world_error(pose, xyz, hits):
    """Distance of pose·xyz to the world hits."""
    p = np.asarray(xyz, np.float64)[:, :3]
    return np.linalg.norm(p @ pose[:3, :3].T + pose[:3, 3] - hits, axis=1)
