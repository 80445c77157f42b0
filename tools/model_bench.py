"""Scan-to-model odometry against the raw FIFO at the same queue size: one pre-generated HDL-64
stream (held in memory, the filtered cloud = the raw sweep, the flat cloud = a random subsample) run
through LaserOdometry at max_queue_size 10, map_model "raw" and "compensated" in alternated rounds in
one process on one GPU.

    python tools/model_bench.py [--frames 12] [--rounds 3] [--queue 10] [--flat 2000] [--out FILE.json]

Per model (median over rounds; every round's figures are kept): frames/s of the whole process() loop;
the wall time of the map push (pack, upload, NaN filter — for "compensated" with the transform fused
into its scatter pass — and the index build: LaserOdometry's push returns the map's size, so it is
synchronous); the index build's device time per push from imls_kernel_timing kind 1 (measured in a
second pass with the timing events on: they change the launch sequence, so that pass gives no
frames/s); ICP iterations per frame; the trajectory RMSE against the generator's ground truth.
Prints one JSON line.  No threshold: the expectation is the same incremental index cost for both
models and nothing measurable for the fused transform.

    python tools/model_bench.py --map-model {voxel,compensated,raw} [--frames 12] [--queue 10] [--out FILE.json]

One model alone in the process ("voxel": the voxel map, which ignores --queue): per frame the wall time
of process(), the device time of the map's update (imls_kernel_timing kind 14) and of the index build
(kind 1), and the map's size."""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--queue", type=int, default=10)
    ap.add_argument("--flat", type=int, default=2000)
    ap.add_argument("--model", default="hdl64", choices=["hdl64", "vlp16"])
    ap.add_argument("--out", default=None)
    ap.add_argument("--map-model", default=None, choices=["raw", "compensated", "voxel"],
                    help="one model alone, per frame: update (kind 14), index (kind 1) and frame time, map size")
    a = ap.parse_args()

    import torch                       # first: the process's HIP runtime (as bench.py)
    if not torch.cuda.is_available():
        raise SystemExit("model_bench: no GPU visible (no CPU fallback)")
    import plo_amd
    plo_amd.load()
    from planetary_lidar_odometry_amd import _abi, config, imls_icp, synth

    sm = synth.hdl64() if a.model == "hdl64" else synth.vlp16()
    scene = synth.make_scene(1)
    traj = [np.asarray(T, dtype=np.float64) for T in synth.trajectory(a.frames + 5, 2001)]
    scans = [synth.scan(scene, sm, traj[5 + k], seed=3000 + k) for k in range(a.frames)]
    rng = np.random.default_rng(7)     # (a seeded random subsample: FPS of a 126k-point sweep takes seconds)
    frames = [(s, s[np.sort(rng.choice(len(s), min(a.flat, len(s)), replace=False))]) for s in scans]
    truth = [np.linalg.inv(traj[5]) @ traj[5 + k] for k in range(a.frames)]

    p = config.params_from_config(config.load())
    p.solve_method = _abi.IMLS_SOLVE_LS
    p.max_queue_size = a.queue

    def run(model, timing):
        push_ms = []
        with imls_icp.LaserOdometry(p, device=0, map_model=model) as lo:
            ctx = lo.ctx
            if timing:
                ctx.enable_timing(1)
                ctx.reset_timing()
            plain_push = ctx.map_push

            def timed_push(cloud, count=True, pose=None):
                t = time.perf_counter()
                r = plain_push(cloud, count=count, pose=pose)
                push_ms.append((time.perf_counter() - t) * 1e3)
                return r

            ctx.map_push = timed_push
            t0 = time.perf_counter()
            for filtered, flat in frames:
                lo.process(filtered, flat)
            wall = time.perf_counter() - t0
            index = ctx.kernel_timing(1) if timing else (0.0, 0)
            iters = [r[2] for r in lo.results]
            err = [np.linalg.norm(now[:3, 3] - truth[k + 1][:3, 3]) for k, (_, now) in enumerate(lo.poses)]
        return dict(fps=len(frames) / wall, push_ms=statistics.median(push_ms[1:]), iters=iters,
                    index_ms=index[0] / max(index[1], 1), index_builds=int(index[1]),
                    rmse=float(np.sqrt(np.mean(np.square(err)))))

    def per_frame(model):
        """One model alone: per frame the wall time of process() (timing off), and in a second pass with
        the timing events on the device time of the map's update (kind 14, the voxel map only) and of the
        index build (kind 1) of that frame's push — both are harvested by the next frame's registration,
        so the last frame's push is not reported — and the map's size after the frame."""
        out = {}
        for timing in (False, False, True):        # the first pass warms up
            wall, sizes, cum = [], [], []
            with imls_icp.LaserOdometry(p, device=0, map_model=model) as lo:
                ctx = lo.ctx
                if timing:
                    ctx.enable_timing(1)
                    ctx.reset_timing()
                for filtered, flat in frames:
                    t = time.perf_counter()
                    lo.process(filtered, flat)
                    wall.append((time.perf_counter() - t) * 1e3)
                    sizes.append(int(ctx.n_target or 0))
                    cum.append((ctx.kernel_timing(14)[0], ctx.kernel_timing(1)[0]))
                err = [np.linalg.norm(now[:3, 3] - truth[k + 1][:3, 3]) for k, (_, now) in enumerate(lo.poses)]
                infos = list(lo.map_infos)
            if not timing:
                out.update(frame_ms=[round(w, 3) for w in wall], map_points=sizes,
                           rmse_m=round(float(np.sqrt(np.mean(np.square(err)))), 5))
                if infos:
                    out["voxels"] = [i["voxels"] for i in infos]
            else:
                d = np.diff(np.asarray([(0.0, 0.0)] + cum), axis=0)[1:]
                out.update(update_ms=[round(float(v), 4) for v in d[:, 0]], index_ms=[round(float(v), 4) for v in d[:, 1]])
        return out

    if a.map_model:
        res = dict(tool="model_bench", map_model=a.map_model, sensor=a.model, frames=a.frames, queue=a.queue,
                   flat_points=a.flat, scan_points=int(np.mean([len(s) for s in scans])), **per_frame(a.map_model))
        line = json.dumps(res)
        print(line)
        if a.out:
            pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            pathlib.Path(a.out).write_text(line + "\n")
        return

    models = ("raw", "compensated")
    for m in models:                   # warm-up: buffers grown, code objects loaded
        run(m, False)
    rounds = {m: [] for m in models}
    for r in range(a.rounds):
        for m in (models if r % 2 == 0 else models[::-1]):
            plain, timed = run(m, False), run(m, True)
            rounds[m].append(dict(fps=round(plain["fps"], 2), push_wall_ms=round(plain["push_ms"], 4),
                                  index_ms_per_push=round(timed["index_ms"], 4), index_builds=timed["index_builds"],
                                  iters=plain["iters"], rmse_m=round(plain["rmse"], 5)))

    def med(m, k):
        return round(statistics.median(x[k] for x in rounds[m]), 4)

    res = dict(tool="model_bench", sensor=a.model, frames=a.frames, queue=a.queue, flat_points=a.flat,
               scan_points=int(np.mean([len(s) for s in scans])), rounds=a.rounds,
               summary={m: dict(fps=med(m, "fps"), push_wall_ms=med(m, "push_wall_ms"),
                                index_ms_per_push=med(m, "index_ms_per_push"), iters=rounds[m][0]["iters"],
                                rmse_m=rounds[m][0]["rmse_m"]) for m in models},
               per_round=rounds)
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
