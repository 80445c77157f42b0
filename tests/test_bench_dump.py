"""CPU: bench.py's --dump-outputs writer (bench.dump_outputs) — the tagged results of one step, here
real registrations of a small golden pair by the CPU oracle, come back from the .npy files ordered
by context, float64, every trace field in place and shorter traces NaN-padded."""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))


def test_dump_outputs_roundtrip(tmp_path):
    import bench
    import oracle_ctypes as oc
    from planetary_lidar_odometry_amd import config
    g = dict(np.load(ROOT / "tests" / "golden" / "vlp16_pair.npz"))
    runs = [oc.register_frame(g["src"], g["tgt"], config.bench_params(it)) for it in (3, 2)]
    # as the timed path tags them: (context, pose, iterations, status, trace), here out of order
    last = [(1, runs[1]["pose"], runs[1]["iters"], runs[1]["status"], runs[1]["trace"]),
            (0, runs[0]["pose"], runs[0]["iters"], runs[0]["status"], runs[0]["trace"])]
    out = tmp_path / "nested" / "dump"
    bench.dump_outputs(out, last)
    got = {f.stem: np.load(f) for f in out.glob("*.npy")}
    assert sorted(got) == ["context", "iterations", "pose", "status", "trace_delta", "trace_n_kept",
                           "trace_n_valid", "trace_pose", "trace_reject"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["context"].tolist() == [0.0, 1.0]
    assert got["iterations"].tolist() == [3.0, 2.0]
    assert got["trace_delta"].shape == (2, 3, 4, 4) and got["trace_n_valid"].shape == (2, 3)
    for k, r in enumerate(runs):
        assert np.array_equal(got["pose"][k], r["pose"])
        assert got["status"][k] == r["status"]
        for j, t in enumerate(r["trace"]):
            assert np.array_equal(got["trace_delta"][k, j].ravel(), np.array(t.delta[:]))
            assert np.array_equal(got["trace_pose"][k, j].ravel(), np.array(t.pose[:]))
            assert got["trace_reject"][k, j].tolist() == [float(v) for v in t.reject]
            assert got["trace_n_valid"][k, j] == t.n_valid and got["trace_n_kept"][k, j] == t.n_kept
    # the 2-iteration registration's third trace slot is padding
    assert np.isnan(got["trace_delta"][1, 2]).all() and np.isnan(got["trace_n_valid"][1, 2])
    assert np.isfinite(got["trace_delta"][0]).all()
    # written again with the same results: identical files
    bench.dump_outputs(out, last)
    assert all(np.array_equal(np.load(out / f"{n}.npy"), a, equal_nan=True) for n, a in got.items())
