"""Kind-13 (pose-info kernels) time per frame next to the frame's registration (HIP events, timing
kinds 0, 2 and 13), capture off and on: a lone config-C frame (2,000 FPS points of a VLP-16 scan) and a
config-B pair (a full HDL-64 scan), LS and the shipped RANSAC → DRPM, 20 registrations each after 3 of
warm-up.  The wall clock is taken with the timing events on.

    python tools/pose_info_probe.py [OUT.json]
"""
import json, sys, time, pathlib
ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import torch  # noqa
import plo_amd
plo_amd.load()
import numpy as np
from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth

out = {}
for name, model, nq in (("config_C_lone_frame", "vlp16", 2000), ("config_B_pair", "hdl64", 0)):
    pair = synth.make_pair(model, map_scans=1, start=5) if model == "vlp16" else synth.make_pair(model, map_scans=1)
    src = synth.fps_subsample(pair.source, nq, seed=1) if nq else pair.source
    for solver in ("LS", "RANSAC_DRPM"):
        p = config.params_from_config(config.load())
        if solver == "LS":
            p.solve_method = _abi.IMLS_SOLVE_LS
        rec = {}
        for on in (False, True):
            with imls_icp.ImlsContext(p) as c:
                c.capture_pose_info(on)
                c.set_target(pair.target)
                c.set_source(src)
                for _ in range(3):
                    c.seed_rng(p.ransac_seed); r = c.register_frame()
                c.enable_timing(1); c.reset_timing()
                wall = []
                for _ in range(20):
                    c.seed_rng(p.ransac_seed)
                    t = time.perf_counter(); r = c.register_frame(); wall.append((time.perf_counter() - t) * 1e3)
                k = {kind: c.kernel_timing(kind) for kind in (0, 2, 13)}
                rec["on" if on else "off"] = dict(
                    wall_ms_median=round(float(np.median(wall)), 4), iters=r["iters"],
                    project_ms=round(k[0][0] / 20, 4), solve_ms=round(k[2][0] / 20, 4),
                    pose_info_ms=round(k[13][0] / 20, 5), pose_info_launches=k[13][1] / 20,
                    n_rows=int(r["info"]["n_rows"]) if on else None,
                    n_valid=int(r["trace"][-1].n_valid) if r["trace"] else None)
        out[f"{name}/{solver}"] = rec
print(json.dumps(out))
if len(sys.argv) > 1:
    pathlib.Path(sys.argv[1]).write_text(json.dumps(out, indent=1) + "\n")
