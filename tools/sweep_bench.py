"""A raw sweep to a pose, two ways, on one pre-generated HDL-64 raw-sweep stream held in memory:

  (a) ScanRegistration.process_raw + LaserOdometry.process — every cloud through host memory;
  (b) LaserOdometry.process_sweep — the clouds stay in HBM (imls_sweep_process).

    python tools/sweep_bench.py [--frames 12] [--warmup 2] [--rounds 3] [--paths ab] [--deskew] [--pose-info] [--out FILE.json]

Both paths run in alternated rounds in one process on one GPU, for the LS solver and the shipped
RANSAC→DRPM.  Per path and solver: the median over the rounds of each round's median ms per frame
(host clock around calls that end in a stream synchronisation; the warm-up frames of every run are
dropped) and the round-to-round spread (max − min of the round medians); the producer's share of that
time; the transfer figures of imls_sweep_info (path (b); path (a) has no such accounting: "not
measured"); and the device time per frame of timing kinds 5, 6, 7, 9, 10, 11 and 12 from a second pass
with the timing events on (that pass gives no ms per frame).  Prints one JSON line.
--deskew runs the same sweeps with a fixed motion (1 m and 3° per sweep) given to both paths, so the
deskew kernel runs in every sweep (the stream itself is generated from a sensor at rest in each sweep:
this times the launch, it does not improve these clouds).  "geometry" (always): one MOVING sweep of the
sensor model, its filtered cloud (front end → [deskew with the true motion] → ring PCA rows) expressed
in the sweep-end frame against the generator's world hits — max and median distance in metres, with
and without the deskew.
--pose-info runs the same passes with the covariance / degeneracy report captured for every frame
(LaserOdometry(pose_info=True)); the timing pass then also gives kind 13 (the pose-info kernels) per frame,
read from the driver's contexts.
--paths a runs the comparator alone (e.g. against another build of the library through
IMLS_LIB_PATH)."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

KINDS = {5: "k_ring_pca", 6: "k_major_avg", 7: "front_end", 9: "three_axis", 10: "curvature", 11: "sweep_kernels",
         12: "deskew"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--paths", default="ab", choices=["ab", "a", "b"])
    ap.add_argument("--model", default="hdl64", choices=["hdl64", "vlp16"])
    ap.add_argument("--deskew", action="store_true", help="a fixed motion set for every sweep (both paths)")
    ap.add_argument("--pose-info", action="store_true", help="capture the pose-info report of every frame")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch                       # first: the process's HIP runtime (as bench.py)
    if not torch.cuda.is_available():
        raise SystemExit("sweep_bench: no GPU visible (no CPU fallback)")
    import plo_amd
    plo_amd.load()
    from planetary_lidar_odometry_amd import _abi, config, imls_icp, producer, synth

    sm = synth.hdl64() if a.model == "hdl64" else synth.vlp16()
    fp = _abi.default_front_params(64 if a.model == "hdl64" else 16)
    if a.model == "vlp16":
        fp.minimum_range, fp.maximum_range = 0.5, 100.0
    scene = synth.make_scene(1)
    total = a.frames + a.warmup
    traj = synth.trajectory(total + 5, 2001)
    raws = [synth.raw_sweep(scene, sm, traj[5 + k], 3000 + k, start_deg=23.0 * k, n_nan=7, n_close=5) for k in range(total)]
    import math
    motion = synth.pose_xyyaw(1.0, 0.05, math.radians(3.0), 0.01, 0.002, 0.004)
    given = motion if a.deskew else None

    def geometry():
        """The filtered cloud of one moving sweep against the generator's world hits."""
        raw, hits, _ = synth.raw_sweep_moving(scene, sm, traj[5], motion, 2999, start_deg=11.0, return_hits=True)
        end = traj[5] @ motion
        out = dict(motion="1 m, 3 deg per sweep", raw_points=len(raw))
        with imls_icp.ImlsContext(device=0) as ctx:
            xyz, inten, idx, sizes = ctx.scan_front_end(raw, fp)
            for name in ("as_delivered", "deskewed"):
                pts = xyz if name == "as_delivered" else ctx.deskew(np.c_[xyz, inten], motion, "end", fp.scan_period)[:, :3]
                rows = ctx.ring_normals_pca(np.ascontiguousarray(pts), sizes)["index"].astype(np.int64)
                q = pts[rows].astype(np.float64) @ end[:3, :3].T + end[:3, 3]
                d = np.linalg.norm(q - hits[idx[rows]], axis=1)
                out[name] = dict(points=len(rows), max_m=round(float(d.max()), 5), median_m=round(float(np.median(d)), 5))
        return out

    def params(solver):
        p = config.params_from_config(config.load())
        if solver == "ls":
            p.solve_method = _abi.IMLS_SOLVE_LS
        return p

    def run(path, solver, timing):
        """One pass over the stream → per-frame ms (total, producer), sweep infos, kernel times, poses."""
        sr = producer.ScanRegistration(shuffle_seed=4, rand_seed=2)
        ms, prod, infos = [], [], []
        with imls_icp.LaserOdometry(params(solver), device=0, producer=sr if path == "b" else None,
                                    pose_info=a.pose_info) as lo:
            if timing:
                sr.ctx.enable_timing(1)
                sr.ctx.reset_timing()
                if a.pose_info:
                    lo.apply(lambda c: c.enable_timing(1))
            if path == "b":
                plain = sr.process_raw_device

                def timed(raw, front_params=None, **kw):
                    t = time.perf_counter()
                    h = plain(raw, front_params, **kw)
                    prod.append((time.perf_counter() - t) * 1e3)
                    infos.append(h.info)
                    return h

                sr.process_raw_device = timed
            for k, raw in enumerate(raws):
                t0 = time.perf_counter()
                if path == "a":
                    cloud, flat = sr.process_raw(raw, fp, motion=given)
                    prod.append((time.perf_counter() - t0) * 1e3)
                    lo.process(cloud, flat, str(k))
                else:
                    lo.process_sweep(raw, str(k), fp, motion=given)
                ms.append((time.perf_counter() - t0) * 1e3)
            kern = {}
            if timing:
                for kind, name in KINDS.items():
                    try:
                        t, n = sr.ctx.kernel_timing(kind)
                    except _abi.ImlsError:         # a library built before this kind existed
                        kern[name] = "not measured"
                        continue
                    kern[name] = dict(ms_per_frame=round(t / total, 4), launches_per_frame=round(n / total, 2))
                if a.pose_info:
                    tn = [c.kernel_timing(13) for c in lo.contexts]
                    kern["pose_info"] = dict(ms_per_frame=round(sum(t for t, _ in tn) / total, 4),
                                             launches_per_frame=round(sum(n for _, n in tn) / total, 2))
            poses = [now.tobytes() for _, now in lo.poses]
            iters = [r[2] for r in lo.results]
        sr.close()
        w = a.warmup
        return dict(ms=ms[w:], prod=prod[w:], infos=infos[w:], kern=kern, poses=poses, iters=iters)

    paths = list(a.paths)
    solvers = ("ls", "ransac_drpm")
    res = dict(tool="sweep_bench", sensor=a.model, frames=a.frames, warmup=a.warmup, rounds=a.rounds,
               raw_points=int(np.mean([len(r) for r in raws])), deskew=bool(a.deskew), pose_info=bool(a.pose_info),
               solvers={})
    for solver in solvers:
        for pth in paths:              # warm-up: buffers grown, code objects loaded
            run(pth, solver, False)
        rounds = {pth: [] for pth in paths}
        last = {}
        for r in range(a.rounds):
            for pth in (paths if r % 2 == 0 else paths[::-1]):
                o = last[pth] = run(pth, solver, False)
                rounds[pth].append(dict(ms_per_frame=round(statistics.median(o["ms"]), 4),
                                        producer_ms=round(statistics.median(o["prod"]), 4),
                                        frame_ms=[round(x, 3) for x in o["ms"]]))
        out = {}
        for pth in paths:
            meds = [x["ms_per_frame"] for x in rounds[pth]]
            pm = statistics.median(x["producer_ms"] for x in rounds[pth])
            timed = run(pth, solver, True)
            d = dict(ms_per_frame=round(statistics.median(meds), 4), spread_ms=round(max(meds) - min(meds), 4),
                     producer_ms=round(pm, 4), producer_share=round(pm / statistics.median(meds), 4),
                     kernels=timed["kern"], iters=last[pth]["iters"], per_round=rounds[pth])
            if pth == "b":
                inf = last[pth]["infos"]
                d["transfers"] = {k: int(statistics.median(i[k] for i in inf)) for k in ("bytes_h2d", "bytes_d2h", "host_syncs")}
                d["transfers"]["raw_bytes"] = int(statistics.median(r.nbytes for r in raws[a.warmup:]))
                d["counts"] = {k: int(statistics.median(i[k] for i in inf)) for k in ("n_front", "n_filtered", "n_candidates", "n_flat")}
            else:
                d["transfers"] = "not measured"
            out[pth] = d
        if len(paths) == 2:
            out["poses_bit_equal"] = last["a"]["poses"] == last["b"]["poses"]
            out["b_below_a_by_more_than_spread"] = bool(
                out["a"]["ms_per_frame"] - out["b"]["ms_per_frame"] > max(out["a"]["spread_ms"], out["b"]["spread_ms"]))
        res["solvers"][solver] = out
    res["geometry"] = geometry()       # after the timed passes: its context and buffers are not part of them
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
