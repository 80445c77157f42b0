"""The three loop solvers side by side — trimmed LS, the robust M-estimator solve and the shipped
RANSAC → DRPM — on one frame alone and on one config-B pair, alternated round by round in one process
on one GPU.

    python tools/solve_bench.py [--methods LS,Robust,RANSAC] [--rounds 7] [--reps 10] [--out FILE.json]

lone frame   the stream workload's frame shape: an HDL-64 sweep through the GPU producer, the flat cloud
             (≤ 2000 points) of frame k + 1 registered against the filtered cloud of frame k
             (max_queue_size 1), host inputs, one context, shipped convergence thresholds.
config B     one HDL-64 scan against a 10-scan map (synth.make_pairs), every point a query.

Per method and case: ms per frame — the median over the rounds of each round's median over --reps
registrations (set_source + register_frame, the map already indexed) — with the rounds' minimum and
maximum; the ICP iterations run; and the solve kernels' share of the device time, from the context's
kernel timing (kind 2 against kinds 0 + 2) in a separate pass with the timing events on (they change
the launch sequence, so that pass gives no ms per frame).  --methods lets a tree without the robust
solve (IMLS_LIB_PATH: another build of the library) run LS and RANSAC alone.  Prints one JSON line."""
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
    ap.add_argument("--methods", default="LS,Robust,RANSAC")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch                       # first: the process's HIP runtime (as bench.py)
    if not torch.cuda.is_available():
        raise SystemExit("solve_bench: no GPU visible (no CPU fallback)")
    import plo_amd
    plo_amd.load()
    from planetary_lidar_odometry_amd import _abi, config, imls_icp, producer, synth

    methods = [m for m in a.methods.split(",") if m]
    ids = {"LS": _abi.IMLS_SOLVE_LS, "Robust": _abi.IMLS_SOLVE_ROBUST, "RANSAC": _abi.IMLS_SOLVE_RANSAC}

    def params(method):
        p = config.params_from_config(config.load())
        p.solve_method = ids[method]
        p.max_queue_size = 1
        return p

    sm = synth.hdl64()
    scene = synth.make_scene(0)
    poses = synth.trajectory(5, 2000)
    with imls_icp.ImlsContext(device=0) as pctx:
        sr = producer.ScanRegistration(ctx=pctx, shuffle_seed=0, rand_seed=1)
        produced = []
        for k in range(2):
            xyz, sizes, inten = producer.sweep_inputs(synth.scan(scene, sm, poses[3 + k], seed=5000 + k), len(sm.rings))
            produced.append(sr.process(xyz, sizes, inten))
    pair = synth.make_pairs(1, "hdl64", map_scans=10, scene_seed=0, traj_seed=2000, noise_seed=1000)[0]
    cases = {"lone_frame": (produced[1][1], produced[0][0]), "config_b_pair": (pair.source, pair.target)}

    ctxs = {}
    for case, (src, tgt) in cases.items():
        for m in methods:
            c = imls_icp.ImlsContext(params(m), device=0)
            c.set_target(tgt)
            ctxs[case, m] = c

    def frame(case, m):
        c = ctxs[case, m]
        if m == "RANSAC":
            c.seed_rng(c.params.ransac_seed)      # every registration draws the same hypotheses
        c.set_source(cases[case][0])
        return c.register_frame()

    def timed(case, m, reps):
        ms = []
        for _ in range(reps):
            t = time.perf_counter()
            r = frame(case, m)
            ms.append((time.perf_counter() - t) * 1e3)
        return statistics.median(ms), r["iters"]

    rounds = {k: [] for k in ctxs}
    iters = {}
    for case in cases:
        reps = a.reps if case == "lone_frame" else max(a.reps // 3, 2)
        for m in methods:                  # warm-up: buffers grown, code objects loaded
            timed(case, m, 2)
        for r in range(a.rounds):
            for m in (methods if r % 2 == 0 else methods[::-1]):
                ms, it = timed(case, m, reps)
                rounds[case, m].append(ms)
                iters[case, m] = it
    share = {}
    for (case, m), c in ctxs.items():
        c.enable_timing(1)
        c.reset_timing()
        for _ in range(3):
            frame(case, m)
        proj, solve = c.kernel_timing(0)[0], c.kernel_timing(2)[0]
        share[case, m] = dict(solve_ms=solve / 3, project_ms=proj / 3, solve_share=solve / max(proj + solve, 1e-30))
        c.enable_timing(0)
        c.close()

    res = dict(tool="solve_bench", rounds=a.rounds, reps=a.reps, methods=methods,
               sizes={case: dict(queries=int(len(src)), map_points=int(len(tgt))) for case, (src, tgt) in cases.items()})
    for case in cases:
        res[case] = {m: dict(ms_per_frame=round(statistics.median(rounds[case, m]), 4),
                             round_min=round(min(rounds[case, m]), 4), round_max=round(max(rounds[case, m]), 4),
                             iterations=int(iters[case, m]), solve_ms=round(share[case, m]["solve_ms"], 4),
                             project_ms=round(share[case, m]["project_ms"], 4),
                             solve_share=round(share[case, m]["solve_share"], 4)) for m in methods}
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
