"""Times the public kNN query (imls_knn_device, timing kind 8) on the config-B shape and, in the
same process on the same queries, imls_project's projection kinds at the identity pose — the
yardstick the kNN figure is reported against (no threshold: the export does less arithmetic than
k_finish but writes 12·k bytes per query where the projection writes 48).

    python tools/knn_bench.py [--k 20] [--r 3.0] [--reps 20] [--map-scans 10] [--out FILE.json]

Prints one JSON line: per-call milliseconds of kind 8 (traversal + export + exact fallback; the
queries' ordering is outside it, as the source's ordering is outside kind 0), the wall time of a
knn_device call sequence, and the projection kinds 0 (all), 3 (k_knn_wave), 4 (k_finish)."""
import argparse
import json
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--r", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--map-scans", type=int, default=10)
    ap.add_argument("--no-self", action="store_true", help="drop self matches (default: ALLOW_SELF_MATCH)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch                       # first: the process's HIP runtime (as bench.py)
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: no GPU visible (the kNN path has no CPU fallback)")
    dev = torch.device("cuda:0")
    import plo_amd
    plo_amd.load()
    from planetary_lidar_odometry_amd import config, imls_icp, synth

    pair = synth.make_pair("hdl64", map_scans=a.map_scans)
    src = pair.source[np.isfinite(pair.source["x"]) & np.isfinite(pair.source["y"]) & np.isfinite(pair.source["z"])]
    nq = len(src)
    q3 = torch.from_numpy(np.ascontiguousarray(synth.soa(src)[:3])).to(dev).contiguous()
    idx = torch.empty((nq, a.k), dtype=torch.int32, device=dev)
    d2 = torch.empty((nq, a.k), dtype=torch.float64, device=dev)
    found = torch.empty(nq, dtype=torch.int32, device=dev)

    p = config.bench_params(1)
    p.search_number = a.k
    p.r = a.r
    with imls_icp.ImlsContext(p, device=0) as c:
        M = c.set_target(pair.target)
        c.set_source(src)
        eye = np.eye(4)

        def knn_call():
            c.knn_device(q3.data_ptr(), nq, a.k, a.r, not a.no_self, idx.data_ptr(), d2.data_ptr(), found.data_ptr())

        for _ in range(3):             # warm-up: buffers grown, code objects loaded
            knn_call()
            c.synchronize()
            c.project(eye)
        c.enable_timing(1)
        c.reset_timing()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            knn_call()
        c.synchronize()
        wall_knn = (time.perf_counter() - t0) / a.reps * 1e3
        for _ in range(a.reps):
            c.project(eye)             # synchronises: the pending kNN events are read here too
        kind = {k: c.kernel_timing(k) for k in (8, 0, 3, 4)}
        c.enable_timing(0)
        nfound = int(found.sum().item())

    def per(k):
        ms, n = kind[k]
        return round(ms / max(n, 1), 4), int(n)

    res = dict(tool="knn_bench", shape=f"hdl64 map_scans={a.map_scans}", target_points=int(M), queries=int(nq), k=a.k,
               r=a.r, allow_self_match=not a.no_self, reps=a.reps, mean_found=round(nfound / nq, 3),
               knn_ms_per_call=per(8)[0], knn_calls=per(8)[1], knn_wall_ms_per_call=round(wall_knn, 4),
               projection_ms_per_call=per(0)[0], projection_calls=per(0)[1],
               k_knn_wave_ms=per(3)[0], k_finish_ms=per(4)[0],
               knn_Mqueries_per_s=round(nq / max(per(8)[0], 1e-9) / 1e3, 2),
               bytes_out_per_query=12 * a.k + 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        pathlib.Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
