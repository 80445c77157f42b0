"""Upstream producer for the registration path: scan_registration.cpp's per-sweep chain for the
shipped config (config.json scan_registration: compute_normal_method "pca" → presample_method
"geometric_features" → sample_method "major_axis") and the other configurations the reference marks
as verified (presample_method "curvature"; sample_method "normal", "three_axis", "random"), on the
GPU through the C ABI.

  ScanRegistration.process_raw(raw) the whole handler: scan_front_end (NaN / range filter, ring
                                    assignment and relative time, 862-1069) → process
  ScanRegistration.process(sweep)   laserCloudHandler's tail (scan_registration.cpp:1136-1229 normals,
                                    1448-1461 + 1481-1489 presample, 1494-1503 sampling) → the two
                                    clouds laser_odometry consumes: pcl_cloud (/laser_cloud_filtered,
                                    the map FIFO's input) and pcl_surface_cloud (/laser_cloud_flat,
                                    the registration's source)

  ScanRegistration.process_raw_device(raw)  process_raw with every cloud staying in HBM
                                    (imls_sweep_process): a DeviceSweep handle with the two clouds as
                                    device pointers, for LaserOdometry.process_sweep

process_raw and process_raw_device take motion= (the sensor at the sweep's end in the frame of the
sensor at its start): the sweep is then deskewed to its end frame between the front end and the normals
(imls_deskew / imls_sweep_set_motion; TransformToEnd, laser_odometry.cpp:91-114).

The sweep comes in ring-concatenated order (`laserCloud`, 1064-1069) with the points per scan
line.  Sampling follows samplePointCloud's dispatch (761-806): "major_axis" samples its first frame
with the "normal" method (frame == 1, 783) and every later one against the previous pcl_cloud.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _abi
from .imls_icp import ImlsContext
from .synth import POINT_DTYPE


SAMPLE_METHODS = ("major_axis", "normal", "three_axis", "random")
PRESAMPLE_METHODS = ("geometric_features", "curvature")


class ScanRegistration:
    def __init__(self, ctx: Optional[ImlsContext] = None, device: int = 0,
                 pca_params: Optional[_abi.ImlsPcaParams] = None, sample_method: str = "major_axis",
                 shuffle_seed: int = 0, rand_seed: int = 1, presample_method: str = "geometric_features",
                 curvature_params: Optional[_abi.ImlsCurvatureParams] = None, points_per_list: int = 200,
                 max_points: int = 2000, normal_params: Optional[_abi.ImlsSampleParams] = None,
                 major_axis_params: Optional[_abi.ImlsSampleParams] = None):
        if sample_method not in SAMPLE_METHODS:
            raise ValueError(f"sample_method {sample_method!r}: the GPU producer ships {', '.join(SAMPLE_METHODS)}")
        if presample_method not in PRESAMPLE_METHODS:
            raise ValueError(f"presample_method {presample_method!r}: the GPU producer ships "
                             f"{', '.join(PRESAMPLE_METHODS)}")
        if not 1 <= int(points_per_list) <= _abi.THREE_AXIS_MAX_POINTS_PER_LIST:
            raise ValueError(f"points_per_list {points_per_list}: must be in [1, {_abi.THREE_AXIS_MAX_POINTS_PER_LIST}]")
        self._own = ctx is None
        self._ctx = ctx                     # an owned context is created at its first use
        self._device = device
        self.pca_params = pca_params if pca_params is not None else _abi.default_pca_params()
        self.sample_method = sample_method
        self.presample_method = presample_method
        self.curvature_params = curvature_params if curvature_params is not None else _abi.default_curvature_params()
        self.points_per_list = int(points_per_list)        # sample_method.three_axis.points_per_list
        self.max_points = int(max_points)                  # sample_method.random.max_points
        self.normal_params = normal_params                 # sample_method.normal / .major_axis blocks
        self.major_axis_params = major_axis_params         # (None: the shipped values)
        self.shuffle_seed = shuffle_seed
        self.rand_seed = rand_seed
        self.frame = 1                      # scan_registration.cpp:64
        self._device_frames = 0             # sweeps run through process_raw_device (the context's counter − 1)
        self.last_xyz: Optional[np.ndarray] = None
        self.last_pca: Optional[dict] = None
        self.last_curvature: Optional[np.ndarray] = None   # per laserCloud point (curvature presample)
        self.last_candidates: Optional[np.ndarray] = None
        self.last_sampled: Optional[np.ndarray] = None

    @property
    def ctx(self) -> ImlsContext:
        if self._ctx is None:
            self._ctx = ImlsContext(device=self._device)
        return self._ctx

    def close(self):
        if self._own and self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def _frame_seed(self) -> int:
        return (self.shuffle_seed + 7919 * self.frame) & 0xFFFFFFFF

    def sample_params(self) -> _abi.ImlsSampleParams:
        first = self.sample_method == "normal" or self.frame == 1
        method = _abi.IMLS_SAMPLE_NORMAL if first else _abi.IMLS_SAMPLE_MAJOR_AXIS
        sp = _abi.default_sample_params(method)
        given = self.normal_params if first else self.major_axis_params
        if given is not None:
            C.memmove(C.byref(sp), C.byref(given), C.sizeof(sp))
            sp.method = method
        sp.shuffle_seed = self._frame_seed()
        sp.rand_seed = (self.rand_seed + self.frame - 1) & 0xFFFFFFFF
        return sp

    def process_raw(self, raw_xyz, front_params: Optional[_abi.ImlsFrontParams] = None, motion=None):
        """The whole laserCloudHandler on a raw sweep (driver order, (n, 3+) float32): the front end
        (NaN / range filter, ring assignment, relative time; 862-1069) then process().  motion (4×4:
        the sensor at the sweep's end in the frame of the sensor at its start): the front end's points
        are deskewed to the sweep-end frame in between (ImlsContext.deskew; TransformToEnd,
        laser_odometry.cpp:91-114), with the relative time the front end computed on the raw points."""
        xyz, inten, _, sizes = self.ctx.scan_front_end(raw_xyz, front_params)
        if motion is not None:
            fp = front_params if front_params is not None else _abi.default_front_params()
            rec = self.ctx.deskew(np.c_[xyz, inten], motion, "end", fp.scan_period)
            xyz, inten = rec[:, :3], rec[:, 3]
        return self.process(xyz, sizes, inten)

    def sweep_params(self, front_params: Optional[_abi.ImlsFrontParams] = None) -> _abi.ImlsSweepParams:
        """This frame's imls_sweep_params: the configured chain with the per-frame seeds of
        sample_params() / _frame_seed()."""
        sp = _abi.default_sweep_params()
        if front_params is not None:
            sp.front = front_params
        sp.pca = self.pca_params
        sp.curvature = self.curvature_params
        if self.normal_params is not None:
            sp.normal = self.normal_params
        if self.major_axis_params is not None:
            sp.major_axis = self.major_axis_params
        sp.presample_method = _abi.PRESAMPLE_IDS[self.presample_method]
        sp.sample_method = _abi.SWEEP_SAMPLE_IDS[self.sample_method]
        sp.points_per_list, sp.max_points = self.points_per_list, self.max_points
        sp.shuffle_seed = self._frame_seed()
        sp.rand_seed = (self.rand_seed + self.frame - 1) & 0xFFFFFFFF
        return sp

    def process_raw_device(self, raw_xyz, front_params: Optional[_abi.ImlsFrontParams] = None, n: Optional[int] = None,
                           stride: int = 3, motion=None) -> "DeviceSweep":
        """process_raw with every cloud staying in HBM (imls_sweep_process): raw_xyz is an (n, 3+)
        float32 array, or a device pointer with n and stride.  A sequence of calls gives the clouds
        the same sequence of process_raw calls gives; do not mix the two on one instance (the
        previous cloud of major_axis lives on the host for one and on the device for the other).
        motion: as process_raw's — set on the context for this sweep (sweep_set_motion), so a later
        call without one is not deskewed."""
        if self.frame != self._device_frames + 1:
            raise RuntimeError("process_raw_device: this instance already ran process / process_raw")
        self.ctx.sweep_set_motion(motion, "end")
        info = self.ctx.sweep_process(raw_xyz, self.sweep_params(front_params), n, stride)
        self.frame += 1
        self._device_frames += 1
        return DeviceSweep(self.ctx, info, self.ctx.sweep_clouds_device())

    def process(self, xyz, ring_sizes, intensity=None):
        """One sweep → (pcl_cloud, pcl_surface_cloud) as POINT_DTYPE arrays (48-byte
        pcl::PointXYZINormal records)."""
        xyz = np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3])
        o = self.ctx.ring_normals_pca(xyz, ring_sizes, self.pca_params)
        idx = o["index"].astype(np.int64)
        cloud = np.zeros(len(idx), POINT_DTYPE)
        cloud["x"], cloud["y"], cloud["z"] = xyz[idx, 0], xyz[idx, 1], xyz[idx, 2]
        cloud["normal_x"], cloud["normal_y"], cloud["normal_z"] = o["normal"][:, 0], o["normal"][:, 1], o["normal"][:, 2]
        if intensity is not None:
            cloud["intensity"] = np.asarray(intensity, np.float32)[idx]
        if self.presample_method == "curvature":           # 1071-1113, 1462-1473, 1481-1489
            curv, cand = self.ctx.presample_curvature(xyz, ring_sizes, o["index"], o["flags"], self.curvature_params)
            cloud["curvature"] = curv[idx]                 # 1220
            self.last_curvature = curv
        else:
            cand = np.nonzero(o["flags"] & _abi.IMLS_PCA_CANDIDATE)[0].astype(np.int32)
        fxyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1)
        if self.sample_method == "three_axis":             # 769-773
            sampled, _ = self.ctx.sample_three_axis(fxyz, o["normal"], o["evals"], cand, self.points_per_list)
        elif self.sample_method == "random":               # 779-781
            sampled = self.ctx.sample_random(cand, self.max_points, self._frame_seed())
        else:
            sampled, _ = self.ctx.sample_point_cloud(fxyz, o["normal"], cand, self.last_xyz, self.sample_params())
        surface = cloud[sampled]
        self.frame += 1
        self.last_xyz = fxyz
        self.last_pca = o
        self.last_candidates = cand
        self.last_sampled = sampled
        return cloud, surface


class DeviceSweep:
    """One sweep's clouds in HBM (ScanRegistration.process_raw_device): device pointers of the
    filtered and flat clouds (SoA float32[6][n]) with their counts, the filtered cloud's intensity and
    curvature arrays, and imls_sweep_info as `info`.  Valid until the second-next sweep on the
    producer's context; download() must be called before the next one."""

    def __init__(self, ctx: ImlsContext, info: dict, clouds: dict):
        self._ctx = ctx
        self.info = info
        self.sweep = info["sweep"]
        self.filtered, self.n_filtered = clouds["filtered"], clouds["n_filtered"]
        self.flat, self.n_flat = clouds["flat"], clouds["n_flat"]
        self.intensity, self.curvature = clouds["intensity"], clouds["curvature"]
        self.sampled: Optional[np.ndarray] = None

    def download(self):
        """(pcl_cloud, pcl_surface_cloud) as POINT_DTYPE arrays; the sampled rows land in `.sampled`."""
        cloud, _ = self._ctx.sweep_download(0)
        surface, self.sampled = self._ctx.sweep_download(1)
        return cloud, surface


def sweep_inputs(cloud: np.ndarray, n_rings: int):
    """A synth.scan sweep (ring-major POINT_DTYPE, intensity = scanID + 0.1·relTime) as the
    producer's inputs: xyz (n, 3) float32, points per ring, intensity."""
    sizes = np.bincount(np.floor(cloud["intensity"]).astype(np.int64), minlength=n_rings).astype(np.int32)
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float32)
    return xyz, sizes, cloud["intensity"].copy()
