"""LaserOdometry(map_model="compensated"): scan-to-model odometry on a map FIFO kept in one fixed map
frame (posed pushes, each registration started at the scan's predicted pose in that frame), against
the same driver restated on the CPU oracle's step functions (tests/model_restatement.py: drive()).

Fixture: 8 VLP-16 frames (scene 0, trajectory seed 2000, frames 5…12, scan seeds 3000+k), the raw
scan as the filtered cloud and its 1500-point FPS subsample as the flat cloud; shipped parameters.
Tolerances are the project's (tests/test_gpu_stream.py): per-frame rPose and the trajectory RMSE
against the restatement within 1e-6 for LS, 1e-5 through RANSAC→DRPM; iteration counts and statuses
equal; pose-file lines equal to oc.format_pose of the GPU poses.

Discrimination against the raw FIFO: on this fixture the CPU oracle alone gives a trajectory RMSE
against ground truth of 0.00216 m compensated and 0.1308 m raw at queue 3 (a ratio of 60); the GPU
tracks the oracle to 1e-6, so the GPU's compensated RMSE must be at most one tenth of its raw RMSE."""
import numpy as np
import pytest

import model_restatement as mr
import oracle_ctypes as oc
from planetary_lidar_odometry_amd import _abi, config, imls_icp

pytestmark = pytest.mark.gpu
QUEUE = 3


def _params(queue=QUEUE, ls=True):
    p = config.params_from_config(config.load())
    if ls:
        p.solve_method = _abi.IMLS_SOLVE_LS
    p.max_queue_size = queue
    return p


@pytest.fixture(scope="module")
def model():
    """The frames, the ground truth and the oracle side of every configuration, computed once."""
    frames, truth = mr.vlp16_stream(8)
    src = mr.soa6(mr.xyzn(frames[1][1]))
    tgt = mr.soa6(mr.xyzn(frames[0][0]))
    for ls in (True, False):                  # the restated loop is the oracle's, from I
        mr.assert_pinned_to_oracle(src, tgt, _params(1, ls))
    want = {
        "plain": mr.drive(frames, _params()),
        "cv": mr.drive(frames, _params(), prior="constant_velocity"),
        "rebase": mr.drive(frames, _params(), rebase_distance=2.5),
        "ransac": mr.drive(frames[:5], _params(ls=False)),
    }
    return frames, truth, want


def _run(frames, p, tmp_path, name, **kw):
    pose_file = tmp_path / f"{name}.txt"
    with imls_icp.LaserOdometry(p, device=0, pose_file=str(pose_file), **kw) as lo:
        for k, (filtered, flat) in enumerate(frames):
            lo.process(filtered, flat, timestamp=f"{1317384506.0 + 0.1 * k:f}")
        return list(lo.results), list(lo.poses), pose_file.read_text().splitlines(keepends=True), lo.rebases, lo.pipelined


def _check(gpu, want, tol):
    results, poses, lines = gpu[:3]
    assert len(results) == len(want) == len(poses) == len(lines)
    err, prev = [], np.eye(4)
    for (ts, rp, it, st), (ts2, now), (wrp, wit, wst, wnow), line in zip(results, poses, want, lines):
        d = np.abs(rp - wrp).max()
        print(f"{ts}: iters {it}/{wit} status {st}/{wst} |ΔrPose| {d:.3e}")
        assert (it, st) == (wit, wst), (ts, it, st, wit, wst)
        assert d < tol, (ts, d)
        assert np.array_equal(now, oc.chain_pose(prev, rp))
        prev = now
        err.append(np.linalg.norm(now[:3, 3] - wnow[:3, 3]))
        assert line == oc.format_pose(now, ts2)
    rmse = float(np.sqrt(np.mean(np.square(err))))
    print(f"trajectory RMSE vs the restatement {rmse:.3e}")
    assert rmse <= tol, rmse


def test_compensated_ls(model, tmp_path):
    frames, _, want = model
    gpu = _run(frames, _params(), tmp_path, "comp", map_model="compensated")
    assert gpu[3] == 0 and not gpu[4]
    _check(gpu, want["plain"], 1e-6)


def test_compensated_constant_velocity(model, tmp_path):
    frames, _, want = model
    _check(_run(frames, _params(), tmp_path, "cv", map_model="compensated", motion_prior="constant_velocity"),
           want["cv"], 1e-6)
    # the first guess saves iterations on this fixture (the oracle's own count)
    assert sum(w[1] for w in want["cv"]) < sum(w[1] for w in want["plain"])


def test_compensated_with_rebases(model, tmp_path):
    """rebase_distance 2.5 m on a 1 m-per-frame trajectory: the map is re-expressed in the newest
    scan's frame twice within the 8 frames; the restatement applies the same rule."""
    frames, _, want = model
    gpu = _run(frames, _params(), tmp_path, "rebase", map_model="compensated", rebase_distance=2.5)
    assert gpu[3] == 2
    _check(gpu, want["rebase"], 1e-6)


def test_compensated_ransac_drpm(model, tmp_path):
    frames, _, want = model
    _check(_run(frames[:5], _params(ls=False), tmp_path, "ransac", map_model="compensated"), want["ransac"], 1e-5)


def test_compensated_map_beats_the_raw_fifo(model, tmp_path):
    frames, truth, _ = model
    rmse = {}
    for m in ("raw", "compensated"):
        _, poses, _, _, _ = _run(frames, _params(), tmp_path, m, map_model=m)
        rmse[m] = mr.rmse_to([now for _, now in poses], truth)
    print(f"trajectory RMSE vs ground truth at queue {QUEUE}: raw {rmse['raw']:.5f} m, compensated {rmse['compensated']:.5f} m")
    assert rmse["compensated"] <= rmse["raw"] / 10.0, rmse


def test_queue_one_is_unchanged_and_stays_pipelined(model, tmp_path):
    frames, _, _ = model
    raw = _run(frames, _params(1), tmp_path, "q1raw")
    comp = _run(frames, _params(1), tmp_path, "q1comp", map_model="compensated")
    assert raw[4] and comp[4]
    assert len(raw[0]) == len(comp[0]) == len(frames) - 1
    for (t0, p0, i0, s0), (t1, p1, i1, s1) in zip(raw[0], comp[0]):
        assert (i0, s0) == (i1, s1) and np.array_equal(p0, p1)
    assert raw[2] == comp[2]
