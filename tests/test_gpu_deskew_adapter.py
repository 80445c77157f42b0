"""GPU: the C++ adapter's deskew.  A small program written here includes include/imls_icp_hip.hpp,
reads a PointXYZINormal cloud and a motion from raw files, calls imls_hip::deskewCloudHip where
TransformToEnd / TransformToStart stand (laser_odometry.cpp:62-114) and dumps the cloud; it is
compiled with the host g++ against the in-tree libimls_gpu.so (rpath) and run as a child process.
Its records must equal ImlsContext.deskew on the same rows, byte for byte."""
import pathlib
import subprocess

import numpy as np
import pytest

from deskew_cases import MOTION
from planetary_lidar_odometry_amd import imls_icp
from planetary_lidar_odometry_amd.synth import POINT_DTYPE

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parent.parent
LIBDIR = ROOT / "planetary-lidar-odometry_amd" / "csrc"

PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>
#include "imls_icp_hip.hpp"
struct PointXYZINormal { float x, y, z, pad0, normal_x, normal_y, normal_z, pad1, intensity, curvature, pad2, pad3; };
static_assert(sizeof(PointXYZINormal) == 48, "layout");
struct Cloud { std::vector<PointXYZINormal> points; size_t size() const { return points.size(); }
  void push_back(const PointXYZINormal& p) { points.push_back(p); } void clear() { points.clear(); } };
struct Matrix4d { double m[16]; double& operator()(int r, int c) { return m[r * 4 + c]; } };
// usage: deskew_adapter <cloud.bin> <motion.bin> <to_end 0|1> <transform_normal 0|1> <out.bin>
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  auto cloud = std::make_shared<Cloud>();
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  PointXYZINormal p;
  while (std::fread(&p, sizeof p, 1, f) == 1) cloud->push_back(p);
  std::fclose(f);
  Matrix4d T;
  f = std::fopen(argv[2], "rb");
  if (!f || std::fread(T.m, 8, 16, f) != 16) return 3;
  std::fclose(f);
  try {
    imls_hip::deskewCloudHip(cloud, T, std::atoi(argv[3]) != 0, std::atoi(argv[4]) != 0, 0.1f);
  } catch (const std::exception& e) { std::fprintf(stderr, "%s\n", e.what()); return 1; }
  f = std::fopen(argv[5], "wb");
  if (!f) return 3;
  std::fwrite(cloud->points.data(), sizeof p, cloud->size(), f);
  std::fclose(f);
  return 0;
}
'''


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("deskew_adapter")
    src = d / "deskew_adapter.cpp"
    src.write_text(PROGRAM)
    out = d / "deskew_adapter"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", f"-I{ROOT / 'include'}", "-o", str(out), str(src),
                    f"-L{LIBDIR}", "-limls_gpu", f"-Wl,-rpath,{LIBDIR}"], check=True)
    return out


@pytest.mark.parametrize("to_end,transform_normal", [(1, 1), (0, 0)])
def test_adapter_equals_the_context(exe, tmp_path, to_end, transform_normal):
    rng = np.random.default_rng(9)
    n = 777
    cloud = np.zeros(n, POINT_DTYPE)
    for f in POINT_DTYPE.names:
        cloud[f] = rng.normal(size=n)
    cloud["x"], cloud["y"], cloud["z"] = (rng.uniform(-60, 60, n) for _ in range(3))
    cloud["intensity"] = (rng.integers(0, 16, n) + 0.1 * rng.uniform(0, 1, n)).astype(np.float32)
    cloud["y"][11] = np.nan
    cloud.tofile(tmp_path / "cloud.bin")
    np.ascontiguousarray(MOTION, np.float64).tofile(tmp_path / "motion.bin")
    out = tmp_path / "out.bin"
    r = subprocess.run([str(exe), str(tmp_path / "cloud.bin"), str(tmp_path / "motion.bin"), str(to_end),
                        str(transform_normal), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, POINT_DTYPE)
    rec = np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["intensity"]], 1)
    nrm = np.stack([cloud["normal_x"], cloud["normal_y"], cloud["normal_z"]], 1)
    with imls_icp.ImlsContext(device=0) as ctx:
        q, m = ctx.deskew(rec, MOTION, "end" if to_end else "start", 0.1, normals=nrm)
    want = cloud.copy()
    want["x"], want["y"], want["z"] = q[:, 0], q[:, 1], q[:, 2]
    if transform_normal:
        want["normal_x"], want["normal_y"], want["normal_z"] = m[:, 0], m[:, 1], m[:, 2]
    assert got.tobytes() == want.tobytes()
    assert not np.array_equal(got["x"][:10], cloud["x"][:10])
