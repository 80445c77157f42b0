"""Times the upstream producer on the GPU for one synthetic HDL-64 frame pair: ring PCA normals +
presample (imls_ring_normals_pca, k_ring_pca) on both sweeps, then major_axis sampling of frame 1
against frame 0 (imls_sample_point_cloud, k_major_avg + k_fps).  Kernel averages from HIP events on
the context stream (timing kinds 5 and 6); call times include host bookkeeping and PCIe.
usage: python tools/producer_probe.py [reps]
       python tools/producer_probe.py --methods [reps]
--methods: the curvature presample (imls_presample_curvature, timing kind 10) and three_axis
sampling at points_per_list 200 (imls_sample_three_axis, kind 9) on frame 0's PCA outputs — per-call
kernel times from HIP events, reported as median / min / max over the reps (IMLS_LIB_PATH selects
another build of the library for an A/B: run the two alternately)."""
import json, pathlib, sys, time
ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import plo_amd
plo_amd.load()
import numpy as np
from planetary_lidar_odometry_amd import _abi, imls_icp, synth

methods = "--methods" in sys.argv
args = [a for a in sys.argv[1:] if a != "--methods"]
reps = int(args[0]) if args else 10
m = synth.hdl64()
sc = synth.make_scene(0)
frames = []
for k in (0, 1):
    cl = synth.scan(sc, m, synth.pose_xyyaw(k * 1.0, 0, np.radians(0.5 * k)), seed=100 + k)
    sizes = np.bincount(np.floor(cl["intensity"]).astype(np.int64), minlength=len(m.rings))
    frames.append((np.stack([cl["x"], cl["y"], cl["z"]], 1).astype(np.float32), sizes))
if methods:
    import os
    xyz, sizes = frames[0]
    with imls_icp.ImlsContext(device=0) as c:
        r = c.ring_normals_pca(xyz, sizes)
        fxyz = xyz[r["index"]]
        geo = np.nonzero(r["flags"] & _abi.IMLS_PCA_CANDIDATE)[0]
        c.enable_timing(True)
        ms = {9: [], 10: []}
        for k in range(reps + 2):                      # two warm-up calls each
            c.reset_timing()
            curv, cc = c.presample_curvature(xyz, sizes, r["index"], r["flags"])
            s, nan = c.sample_three_axis(fxyz, r["normal"], r["evals"], geo, 200)
            if k >= 2:
                for kind in ms:
                    ms[kind].append(c.kernel_timing(kind)[0])
    stat = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
    print(json.dumps({"lib": os.environ.get("IMLS_LIB_PATH", "default"), "points": int(len(xyz)), "rows": int(len(fxyz)),
                      "geometric_candidates": int(len(geo)), "curvature_candidates": int(len(cc)),
                      "sampled": int(len(s)), "nan_keys": nan, "reps": reps, "three_axis_ms": stat(ms[9]),
                      "curvature_ms": stat(ms[10])}))
    sys.exit(0)
with imls_icp.ImlsContext(device=0) as c:
    def run():
        out = []
        for xyz, sizes in frames:
            r = c.ring_normals_pca(xyz, sizes)
            out.append((xyz[r["index"]], r["normal"], np.nonzero(r["flags"] & _abi.IMLS_PCA_CANDIDATE)[0]))
        (x0, n0, c0), (x1, n1, c1) = out
        t = time.perf_counter()
        s, w = c.sample_point_cloud(x1, n1, c1, x0, _abi.default_sample_params(_abi.IMLS_SAMPLE_MAJOR_AXIS))
        return s, time.perf_counter() - t, len(c1), len(x0)
    for _ in range(2):
        run()
    c.enable_timing(True); c.reset_timing()
    ts = []
    for _ in range(reps):
        s, dt, ncand, mlast = run()
        ts.append(dt)
    pca_ms, pca_n = c.kernel_timing(5)
    avg_ms, avg_n = c.kernel_timing(6)
print(json.dumps({"points": [int(len(f[0])) for f in frames], "candidates": ncand, "last_cloud": mlast,
                  "sampled": int(len(s)), "k_ring_pca_ms": pca_ms / max(pca_n, 1),
                  "k_major_avg_ms": avg_ms / max(avg_n, 1), "sample_call_ms": 1e3 * float(np.median(ts))}))
